"""The inputs of test_wide_nodes_gpu.py reach what that file is about, shown on the C oracle and the host models alone (CPU only):
every condition a GPU test there depends on is counted here, printed, and must be at least 1.  And the oracle itself against the
unmodified reference on wide nodes (tests/golden/mcts_wide.json, written by tests/golden/gen_golden.py --wide-only)."""
import json
import os

import numpy as np
import pytest

import search_edges as E
import searchdrive
import wide_cases as W
from oracle import oracle as O
from test_oracle_golden import _PerTreeOracle
from test_width import _OracleK


def _total(plies):
    c = dict(W.ZERO)
    for p in plies:
        c = W.add(c, p["cond"])
    return c


def _need(c, *keys):
    for k in keys:
        assert c[k] >= 1, (k, c)


def test_roots_are_wide_with_narrow_neighbours(rules_golden):
    boards, side, rr = W.reference_roots(rules_golden)
    w = W.widths(boards, side)
    print("wide roots: %d trees, %d with more than 64 moves, %d with more than 96, widest %d; %d black to move; %d at rr 57"
          % (len(w), (w > 64).sum(), (w > 96).sum(), w.max(), side.sum(), (rr == 57).sum()))
    assert 48 <= len(w) <= 96 and (w > 96).sum() >= 8 and w.max() < W.PLAYOUTS
    assert (w[W.EVERY - 1::W.EVERY] <= 64).all() and 8 <= side.sum() <= len(w) - 8 and (rr == 57).sum() >= 8 and rr.any()


@pytest.mark.parametrize("name,bf16", [("signed", False), ("posabs", False), ("signed", True), ("posabs", True)])
def test_width_1_conditions(rules_golden, name, bf16):
    _, plies = W.reference(rules_golden, name, bf16)
    for ply, p in enumerate(plies):
        print("width 1, %s%s, ply %d: %s" % (name, " rounded to bf16" if bf16 else "", ply, p["cond"]))
        assert not np.any(p["status"][0] & ~2)      # only games that have ended (a root without a move) stop
    c = _total(plies)
    _need(c, "expanded_gt64", "expanded_gt96", "inner_sel_ge64", "inner_sel_ge96")
    if name == "posabs":
        _need(c, "root_sel_ge64", "root_sel_ge96", "played_ge64")
        _need(plies[0]["cond"], "root_sel_ge96", "played_ge64")       # from fresh roots: the first advance keeps a second-round subtree


@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("name", ["signed", "posabs"])
def test_width_k_conditions(rules_golden, name, K):
    _, plies = W.reference_k(rules_golden, name, K)
    for ply, p in enumerate(plies):
        print("width %d, %s, ply %d: %d lock-steps, %s" % (K, name, ply, p["steps"], p["cond"]))
        live = (p["status"][0] & ~8) == 0
        assert np.all(p["status"][2][live] == W.PLAYOUTS)             # the exact budget
    c = _total(plies)
    _need(c, "expanded_gt96", "inner_sel_ge64", "inner_sel_ge96")
    if name == "posabs":
        _need(c, "root_sel_ge64", "root_sel_ge96", "played_ge64")


def test_width_4_with_parked_rows_conditions(rules_golden):
    boards, side, rr = W.reference_roots(rules_golden)
    G = len(boards)
    orc = W.k4_masked_oracle(boards, side, rr)
    E.lockstep(orc, W.K4_STEPS, W.net("signed"), select_args=lambda step: dict(mask=W.k4_mask(G, step)))
    cond = W.conditions(orc.root_stats(), [orc.tree_dump(g) for g in range(G)])
    print("width 4 with parked rows: %s" % cond)
    _need(cond, "expanded_gt96", "inner_sel_ge64")


def test_policy_fc_conditions(rules_golden):
    _, plies = W.reference_fc(rules_golden)
    for ply, p in enumerate(plies):
        print("policy FC inside the expansion, ply %d: %s" % (ply, p["cond"]))
    _need(_total(plies), "expanded_gt96", "inner_sel_ge64")


def test_cache_lenders_are_wide(rules_golden):
    """Transpositions inside the trees of the first ply (before any re-root drops a cache entry): the nodes an evaluation cache can
    expand from a lender, and those of them with more than 64 children."""
    (boards, side, rr), plies = W.reference(rules_golden, "signed")
    D = Wd = 0
    for g in range(len(boards)):
        d, w = W.transpositions(boards[g], side[g], plies[0]["dumps"][g])
        D, Wd = D + d, Wd + w
    print("signed, first ply: %d expanded nodes repeat a position of their tree, %d of them with more than 64 children" % (D, Wd))
    assert Wd >= 1


def test_lines_conditions(rules_golden):
    _, plies = W.reference(rules_golden, "posabs")
    starts, ties, below = W.lines_conditions(plies[0]["stats"], plies[0]["dumps"])
    print("posabs, first ply: %d visited root children of index >= 64, %d trees with equal visit counts across the two rounds, "
          "%d steps of a line into a child of index >= 64 below the root" % (starts, ties, below))
    assert starts >= 1 and ties >= 1 and below >= 1


@pytest.mark.parametrize("rules", ["capture", "xiangqi"])
@pytest.mark.parametrize("sample_plies", [0, 2])
def test_match_conditions(rules_golden, sample_plies, rules):
    op, want, ranks, sampled = W.match_reference(rules_golden, sample_plies, rules)
    plies = want["plies"]
    hi = ranks >= 64
    print("match, rules %s, sample_plies %d: %d choices, of rank >= 64: %d greedy, %d sampled (highest %d); reasons %s"
          % (rules, sample_plies, len(ranks), (hi & ~sampled).sum(), (hi & sampled).sum(), ranks.max(), np.bincount(want["reason"]).tolist()))
    assert (hi & sampled).sum() >= 1 if sample_plies else (hi & ~sampled).sum() >= 1
    assert len(ranks) >= plies.sum() and sampled.any() == bool(sample_plies)
    assert max(p for _, _, p in W.MATCH_PLAYERS) > W.widths(op.boards, op.side).max() > 96


def test_selfplay_conditions(rules_golden):
    roots, want, ranks = W.selfplay_reference(rules_golden)
    print("self-play at the king-safe level: %s; %d picks, %d of rank >= 64 (highest %d), %d plies with an unsafe child, smallest margin %.3g"
          % (want["stats"], want["picks"], (ranks >= 64).sum(), ranks.max(), want["unsafe_plies"], want["min_margin"]))
    assert (ranks >= 64).sum() >= 1 and want["unsafe_plies"] >= 1 and want["min_margin"] >= 1e-12 and want["picks"] == want["stats"]["plies"]


# ---- the oracle against the unmodified reference ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mcts_wide_golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "mcts_wide.json")))


def test_golden_cases_are_wide(mcts_wide_golden):
    cases = mcts_wide_golden["cases"]
    n = [len(c["moves"]) for c in cases]
    movers = {c["plies"][0]["player"] for c in cases}
    root_top = max(p["root_top_index"] for c in cases for p in c["plies"])
    inner_top = max(p["inner_top_index"] for c in cases for p in c["plies"])
    print("mcts_wide.json: %d cases with %s moves at the root; highest selected index %d under a root, %d under another node" % (len(cases), n, root_top, inner_top))
    assert len(cases) == 8 and movers == {"w", "b"} and sum(x > 96 for x in n) >= 2 and min(n) > 64
    assert {c["mode"] for c in cases} == {"signed", "posabs"} and any(len(c["plies"]) == 2 for c in cases)
    assert root_top >= 96 and inner_top >= 96
    for mode in ("signed", "posabs"):
        assert max(p["inner_top_index"] for c in cases if c["mode"] == mode for p in c["plies"]) >= 64, mode


def test_move_lists_match_reference(mcts_wide_golden):
    for c in mcts_wide_golden["cases"]:
        p = c["plies"][0]
        got = O.legal_moves(searchdrive.fen_to_board(p["state"]), 1 if p["player"] == "b" else 0)
        assert got.tolist() == c["moves"], c["name"]


@pytest.mark.parametrize("path", ["width1", "k1"])
def test_search_matches_reference_on_wide_nodes(mcts_wide_golden, path):
    """czo_search_select / czo_search_expand_backup, and the k-wide calls with k = 1, against the reference's trees."""
    cases = mcts_wide_golden["cases"]
    eng = _PerTreeOracle(len(cases)) if path == "width1" else _OracleK(len(cases))
    results, logs = searchdrive.run_cases(eng, cases)
    if path == "width1":
        assert not np.any(eng.status() & ~8)
    searchdrive.check_against_golden(results, logs, cases)
