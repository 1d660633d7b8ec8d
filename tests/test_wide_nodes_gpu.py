"""Nodes of 65-128 children on the device: the second round of 64 lanes in every kernel that walks a node's children — select_body and
k_select_k, the expansion kernels (the in-kernel policy FC included), the lending and filing paths of the evaluation cache, k_lines,
the choose kernels of matches and self-play, the re-root compaction — against the C oracle and the host models, bit for bit: no
tolerance anywhere, floats are compared as their bits.

The inputs and the conditions that prove them are tests/wide_cases.py's; test_wide_nodes_cpu.py asserts every condition on the
oracle alone, each test here names the ones it depends on and asserts them again where it has the oracle's trees at hand."""
import json
import os
import time

import numpy as np
import pytest
import torch

import match_model as MM
import search_edges as E
import searchdrive
import wide_cases as W
from test_hip_lines import _assert_equal as _same_lines, _model as _lines_model
from test_search_edges_gpu import MAXREC, _bits, _Follower, _np, _same_search, _status

pytestmark = pytest.mark.gpu


def _need(c, *keys):
    for k in keys:
        assert c[k] >= 1, (k, c)


def _same_as(eng, ref, what, nodes_too=False):
    """The engine's status, simulation counters, root statistics and EVERY tree against one ply of an oracle run."""
    hst, hnodes, hsims = _status(eng)
    ost, onodes, osims = ref["status"]
    assert np.array_equal(hst, ost) and np.array_equal(hsims, osims), what
    if nodes_too:
        assert np.array_equal(hnodes, onodes), what
    hs, os_ = eng.root_stats_host(), ref["stats"]
    for key in ("label", "N", "count"):
        assert np.array_equal(hs[key], os_[key]), (what, key)
    for key in ("Q", "P", "W"):
        assert np.array_equal(_bits(hs[key]), _bits(os_[key])), (what, key)
    for g in range(len(ost)):
        assert np.array_equal(eng.tree_dump(g, MAXREC), ref["dumps"][g]), (what, g)


def _device_net(fwd):
    def forward(planes):
        lg, v = fwd(_np(planes.float()[..., :14]))
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    return forward


# ---- width 1, every step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,advance,bf16", [("signed", "lds", False), ("posabs", "lds", False), ("posabs", "global", False), ("signed", "global", True)],
                         ids=["signed-lds", "posabs-lds", "posabs-global", "signed-global-bf16"])
def test_width_1_equals_oracle_every_step(rules_golden, name, advance, bf16):
    """63 trees, 3 plies of 1 + 140 lock-steps, the most visited child played.  Planes and needs_eval every step (over stale buffers);
    root statistics, every tree's dump, status and counters after every ply; root_state after every advance, the re-root compaction
    with its bitmap in LDS or in global memory.  bf16: 16-channel bf16 planes, logits and values handed over as bf16.
    Conditions: "signed" — selected children of index >= 64 and >= 96 under non-root parents; "posabs" — selected root children of
    index >= 64 and >= 96, and a played child of index >= 64 out of fresh roots (the advance keeps a second-round subtree)."""
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import SearchEngine
    t0 = time.time()
    boards, side, rr = W.reference_roots(rules_golden)
    G = len(boards)
    eng = SearchEngine(G, W.CAP, plane_dtype=torch.bfloat16, channels=16) if bf16 else SearchEngine(G, W.CAP)
    if advance == "global":
        check(lib().cz_search_debug_advance_in_global_memory(eng.ctx.h, 1), "cz_search_debug_advance_in_global_memory")
    orc = E.OracleSearch(G, W.CAP, 1)
    eng.reset(boards, side, rr)
    orc.reset(boards, side, rr)
    fol, net = _Follower(eng, orc, bf16_inputs=bf16), W.net(name, bf16)
    total = dict(W.ZERO)
    for ply in range(W.PLIES):
        E.lockstep(orc, W.PLAYOUTS + 1, net, fol)
        ref = dict(status=orc.status(), stats=orc.root_stats(), dumps=[orc.tree_dump(g) for g in range(G)])
        _same_as(eng, ref, (name, advance, ply), nodes_too=ply == 0)     # the engine compacts on advance, the oracle does not
        stats = ref["stats"]
        cond = W.conditions(stats, ref["dumps"])
        total = W.add(total, cond)
        if ply == 0 and name == "posabs":
            _need(cond, "root_sel_ge96", "played_ge64")
        played = E.most_visited(stats)
        eng.advance(played)
        orc.advance(played)
        for h, o in zip(eng.root_state(), orc.root_state()):
            assert np.array_equal(_np(h), o), ply
        for g in range(G):
            assert np.array_equal(eng.tree_dump(g, MAXREC), orc.tree_dump(g)), (ply, g)
    _need(total, "expanded_gt96", "inner_sel_ge64", "inner_sel_ge96")
    if name == "posabs":
        _need(total, "root_sel_ge64", "root_sel_ge96", "played_ge64")
    print("width 1, %s, advance %s%s: %s in %.1f s" % (name, advance, ", bf16" if bf16 else "", total, time.time() - t0))


# ---- width k -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16])
@pytest.mark.parametrize("name", ["signed", "posabs"])
def test_width_k_budgeted_search_equals_oracle(rules_golden, name, K):
    """SearchEngine.search(width = K) with its exact budget (cz_search_set_sim_target) against czo_search_select_k under the same
    schedule: 2 plies of exactly 140 simulations per tree, the same number of lock-steps, every tree equal.
    Conditions: selected children of index >= 64 and >= 96 under non-root parents; "posabs": under the root as well, and a played
    child of index >= 64."""
    from cchess_zero_amd.engine import SearchEngine
    t0 = time.time()
    (boards, side, rr), plies = W.reference_k(rules_golden, name, K)
    total = dict(W.ZERO)
    for p in plies:
        total = W.add(total, p["cond"])
    _need(total, "expanded_gt96", "inner_sel_ge64", "inner_sel_ge96")
    if name == "posabs":
        _need(total, "root_sel_ge64", "root_sel_ge96", "played_ge64")
    eng = SearchEngine(len(boards), W.K_CAP, width=K)
    eng.reset(boards, side, rr)
    fwd = _device_net(W.net(name))
    for ply, p in enumerate(plies):
        steps = eng.search(fwd, W.PLAYOUTS)
        assert steps == p["steps"], (ply, steps, p["steps"])
        _same_as(eng, p, (K, name, ply), nodes_too=ply == 0)
        eng.advance(p["played"])
    print("width %d, %s: %s lock-steps, %s in %.1f s" % (K, name, [p["steps"] for p in plies], total, time.time() - t0))


def test_width_4_with_parked_rows_equals_oracle_every_step(rules_golden):
    """k_select_k / k_expand_backup_k at K = 4, every step: from step 1 on tree g sits out the steps with (g + step) % 3 == 0 (one
    oracle search per tree, not called for a masked tree); planes and needs_eval of all 4 rows of every tree over stale buffers.
    Condition: selected children of index >= 64 under non-root parents."""
    from cchess_zero_amd.engine import SearchEngine
    t0 = time.time()
    boards, side, rr = W.reference_roots(rules_golden)
    G = len(boards)
    eng = SearchEngine(G, W.K_CAP, width=4)
    orc = W.k4_masked_oracle(boards, side, rr)
    eng.reset(boards, side, rr)
    E.lockstep(orc, W.K4_STEPS, W.net("signed"), _Follower(eng, orc, per_step=True), select_args=lambda step: dict(mask=W.k4_mask(G, step)))
    stats, _ = _same_search(eng, orc, G)
    cond = W.conditions(stats, [orc.tree_dump(g) for g in range(G)])
    _need(cond, "expanded_gt96", "inner_sel_ge64")
    print("width 4 with parked rows: %s in %.1f s" % (cond, time.time() - t0))


# ---- the policy FC inside the expansion, plain and compact batches ------------------------------------------------------------------
class _FcNet:
    """What SearchEngine.step takes for a fused net: search_eval(planes, n_rows) -> (z [G, 90, 3], value [G, 1]) computed from each
    ROW's planes (so a compact batch, whose row r belongs to whichever tree was handed r, gets that tree's numbers), and the policy
    FC's weights for cz_search_expand_backup_fc."""
    fused_search = True

    def __init__(self, dev):
        w, b = W.fc_weights()
        self.pfc_w_rows, self.pfc_b_f32 = torch.from_numpy(w).to(dev), torch.from_numpy(b).to(dev)

    def search_eval(self, planes, n_rows):
        z, v = W.fc_net(_np(planes.float()[..., :14]))
        return torch.from_numpy(z).to(planes.device), torch.from_numpy(v).to(planes.device)


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
def test_policy_fc_inside_the_expansion_equals_oracle(rules_golden, compact):
    """cz_search_expand_backup_fc — the FC evaluated inside the expansion for the legal moves only, ridx[CZD_MAXMOVES] — against the
    oracle fed the full logits of the same FC restated in NumPy float32 (searchdrive.fc_logits_restated): 24 of the roots, 2 plies
    of 1 + 60 lock-steps.  compact: cz_search_select_compact hands out the net's rows (select_body<COMPACT>).
    Conditions: expansions of more than 96 legal moves; selected children of index >= 64 under non-root parents."""
    from cchess_zero_amd.engine import SearchEngine
    t0 = time.time()
    (boards, side, rr), plies = W.reference_fc(rules_golden)
    total = dict(W.ZERO)
    for p in plies:
        total = W.add(total, p["cond"])
    _need(total, "expanded_gt96", "inner_sel_ge64")
    eng = SearchEngine(len(boards), W.CAP)
    eng.compact = compact
    eng.reset(boards, side, rr)
    net = _FcNet(eng.dev)
    for ply, p in enumerate(plies):
        for step in range(W.FC_STEPS + 1):
            eng.step(net, mode=0 if step == 0 else 1)
        _same_as(eng, p, ("fc", compact, ply), nodes_too=ply == 0)
        eng.advance(p["played"])
    want_rows, tree_steps = sum(p["rows"] for p in plies), W.FC_PLIES * (W.FC_STEPS + 1) * len(boards)
    assert want_rows < tree_steps                      # some leaves are king captures or 60-ply draws: a compact batch is shorter
    if compact:                                        # exactly the rows the oracle's leaves asked for
        assert eng.eval_totals() == (want_rows, W.FC_PLIES * (W.FC_STEPS + 1))
    print("policy FC inside the expansion (%s): %d net rows for %d tree-steps, %s in %.1f s"
          % ("compact" if compact else "plain", want_rows, tree_steps, total, time.time() - t0))


# ---- terminal simulations inside select, the evaluation cache -----------------------------------------------------------------------
def _budgeted_ply(eng, fwd, playouts, extra):
    """One ply with terminal_extra and a budget of exactly `playouts` simulations per tree -> the net rows it used."""
    eng.set_terminal_extra(extra)
    eng.set_sim_target(playouts)
    rows = 0
    try:
        for mode in [0] + [1] * playouts:
            st, _, sims = _status(eng)
            if mode == 1 and not ((sims < playouts) & ((st & ~E.ST_BAD_ADVANCE) == 0)).any():
                break
            planes, need = eng.select(mode)
            rows += int(_np(need).sum())
            lg, v = fwd(_np(planes))
            eng.expand_backup(torch.from_numpy(lg).to(eng.dev), torch.from_numpy(v).to(eng.dev))
    finally:
        eng.set_sim_target(0)
        eng.set_terminal_extra(0)
    return rows


@pytest.mark.parametrize("variant,key_bits,xc,extra", [("extra", 64, 0, 1), ("extra", 64, 0, 3), ("cache", 64, 0, 0), ("cache", 11, 0, 3),
                                                       ("cache", 64, 12, 3), ("cache", 11, 12, 0)],
                         ids=["extra1", "extra3", "cache64", "cache11", "xcache64", "xcache11"])
def test_terminal_extra_and_eval_cache_keep_the_plain_schedules_trees(rules_golden, variant, key_bits, xc, extra):
    """Terminal simulations completing inside select (1 and 3 per launch) and the evaluation cache (64-bit and 11-bit keys, without
    and with the cross-tree level) on the wide roots, "signed", 3 plies of exactly 140 simulations: after every ply every tree,
    statistic and status equals the plain schedule's (the oracle's).
    Condition (cache): a hit whose lender has more than 64 children — in the first ply the oracle's trees hold D expanded nodes
    that repeat a position of their tree, W of them with more than 64 children; each was expanded from the net or from the cache,
    so with H hits at least W - (D - H) hits copied more than 64 children."""
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import SearchEngine
    t0 = time.time()
    (boards, side, rr), plies = W.reference(rules_golden, "signed")
    G = len(boards)
    eng = SearchEngine(G, W.CAP)
    fwd = W.net("signed")
    try:
        if variant == "cache":
            check(lib().cz_search_debug_eval_cache_key_bits(eng.ctx.h, key_bits), "cz_search_debug_eval_cache_key_bits")
            eng.set_eval_cache(True)
            if xc:
                eng.set_xcache(xc)
        eng.reset(boards, side, rr)
        rows, hits0 = 0, None
        for ply, p in enumerate(plies):
            rows += _budgeted_ply(eng, fwd, W.PLAYOUTS, extra)
            _same_as(eng, p, (variant, key_bits, xc, extra, ply), nodes_too=ply == 0)
            if ply == 0 and variant == "cache":
                hits0 = eng.eval_cache_stats()[0]
            eng.advance(p["played"])
        if variant == "cache":
            D = Wd = 0
            for g in range(G):
                d, w = W.transpositions(boards[g], side[g], plies[0]["dumps"][g])
                D, Wd = D + d, Wd + w
            hits, lookups = eng.eval_cache_stats()
            print("evaluation cache, %d-bit keys, cross-tree 2^%d, terminal_extra %d: first ply %d hits for %d repeated positions (%d wide); "
                  "%d hits / %d lookups over 3 plies, %d collisions refused, %s; %d net rows; %.1f s"
                  % (key_bits, xc, extra, hits0, D, Wd, hits, lookups, eng.eval_cache_collisions(), eng.xcache_stats() if xc else "-", rows, time.time() - t0))
            assert hits0 <= D and Wd - (D - hits0) >= 1
            assert (eng.eval_cache_collisions() > 0) if key_bits < 64 else (eng.eval_cache_collisions() == 0)
        else:
            print("terminal_extra %d: %d net rows for %d simulations; %.1f s" % (extra, rows, 3 * W.PLAYOUTS * G, time.time() - t0))
    finally:
        if variant == "cache":
            eng.set_eval_cache(False)
            check(lib().cz_search_debug_eval_cache_key_bits(eng.ctx.h, 64), "cz_search_debug_eval_cache_key_bits")


def test_cross_tree_cache_lends_wide_nodes(rules_golden):
    """The cross-tree level as a lender of more than 64 children (ec_expand_from<XC>, xc_file): every root twice in one engine.  The
    first copies search alone and file what the net gives them; then the second copies search alone — the same positions in the
    same order, so nearly every leaf is lent by the table.  Both halves must equal the oracle's trees.
    Condition: tree g of the second half has W_g expanded nodes of more than 64 children below its root and took R_g net rows, each
    of which expanded one node: at least W_g - R_g wide nodes came out of a cache, and all but H of them — the hits of the per-tree
    level, whatever they lent — out of the cross-tree table."""
    from cchess_zero_amd.engine import SearchEngine
    t0 = time.time()
    (boards, side, rr), plies = W.reference(rules_golden, "signed")
    G, p = len(boards), plies[0]
    eng = SearchEngine(2 * G, W.CAP)
    fwd = W.net("signed")
    try:
        eng.set_eval_cache(True)
        eng.set_xcache(15)
        eng.reset(np.concatenate([boards, boards]), np.concatenate([side, side]), np.concatenate([rr, rr]))
        eng.set_sim_target(W.PLAYOUTS)
        rows = np.zeros((2, 2 * G), np.int64)
        for half in (0, 1):
            mask = (np.arange(2 * G) // G == half).astype(np.uint8)
            for step in range(W.PLAYOUTS + 1):
                planes, need = eng.select(0 if step == 0 else 1, active=mask)
                if step:
                    rows[half] += _np(need)
                lg, v = fwd(_np(planes))
                eng.expand_backup(torch.from_numpy(lg).to(eng.dev), torch.from_numpy(v).to(eng.dev))
        eng.set_sim_target(0)
        hst, _, hsims = _status(eng)
        hs = eng.root_stats_host()
        wide_lent = 0
        for half in (0, 1):
            sl = slice(half * G, (half + 1) * G)
            assert np.array_equal(hst[sl], p["status"][0]) and np.array_equal(hsims[sl], p["status"][2]), half
            for key in ("label", "N", "count"):
                assert np.array_equal(hs[key][sl], p["stats"][key]), (half, key)
            for key in ("Q", "P", "W"):
                assert np.array_equal(_bits(hs[key][sl]), _bits(p["stats"][key])), (half, key)
            for g in range(G):
                assert np.array_equal(eng.tree_dump(half * G + g, MAXREC), p["dumps"][g]), (half, g)
        for g in range(G):
            wide_lent += max(0, int((p["dumps"][g][:, 6] > 64).sum()) - int(rows[1, G + g]))
        st = eng.xcache_stats()
        wide_lent -= eng.eval_cache_stats()[0]
        print("cross-tree cache: net rows %d for the first copies, %d for the second; %s; at least %d nodes of more than 64 children lent; %.1f s"
              % (rows[0].sum(), rows[1].sum(), st, wide_lent, time.time() - t0))
        assert not rows[0, G:].any() and not rows[1, :G].any() and st["hits"] > 0 and rows[1].sum() < rows[0].sum()
        assert wide_lent >= 1
    finally:
        eng.set_sim_target(0)
        eng.set_eval_cache(False)


# ---- principal variations -----------------------------------------------------------------------------------------------------------
def test_lines_of_second_round_children(rules_golden):
    """cz_search_lines with n_lines = 128 on the "posabs" trees of the first ply against lines_model over the same dumps, without and
    with a king-safe candidate mask (the compaction of the candidates runs over both rounds).
    Conditions: lines that start at root children of index >= 64; trees in which the same visit count occurs in both rounds — the
    order of their lines is the model's "earlier first among equals" across the rounds; below the root, a line that steps into a
    most visited child of index >= 64."""
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.rules import Rules
    t0 = time.time()
    (boards, side, rr), plies = W.reference(rules_golden, "posabs")
    G, p = len(boards), plies[0]
    starts, ties, below = W.lines_conditions(p["stats"], p["dumps"])
    assert starts >= 1 and ties >= 1 and below >= 1
    eng = SearchEngine(G, W.CAP)
    eng.reset(boards, side, rr)
    eng.search(_device_net(W.net("posabs")), W.PLAYOUTS)
    dumps = [eng.tree_dump(g, MAXREC) for g in range(G)]
    for g in range(G):
        assert np.array_equal(dumps[g], p["dumps"][g]), g          # the trees the conditions were counted on
    mask = _np(Rules(ctx=eng.ctx).movegen_kingsafe(*eng.root_state()[:2], want_moves=False)[2])
    for n_lines, max_len in ((128, 6), (70, 2)):
        _same_lines(eng.lines_host(n_lines, max_len), _lines_model(dumps, None, n_lines, max_len), ("free", n_lines))
        _same_lines(eng.lines_host(n_lines, max_len, allowed=mask), _lines_model(dumps, mask, n_lines, max_len), ("safe", n_lines))
    free = eng.lines_host(128, 6)
    from_second_round = tied = 0
    for g in range(G):
        n = int(p["stats"]["count"][g])
        index = {int(l): i for i, l in enumerate(p["stats"]["label"][g, :n])}
        first = [index[int(m)] for m, ln in zip(free["moves"][g, :, 0], free["len"][g]) if ln]
        assert sorted(first) == list(range(n)), g                  # with 128 lines every root child starts one
        from_second_round += sum(1 for j, i in enumerate(first) if i >= 64 and free["visits"][g, j, 0] > 0)
        v = free["visits"][g, :len(first), 0]
        tied += sum(1 for j in range(len(first) - 1) if v[j] == v[j + 1] and v[j] > 0 and (first[j] < 64) != (first[j + 1] < 64)
                    and first[j] < first[j + 1])
    print("lines: %d start at a visited root child of index >= 64, %d neighbours in the order tie across the two rounds, %d steps "
          "below the root into a child of index >= 64; %.1f s" % (from_second_round, tied, below, time.time() - t0))
    assert from_second_round == starts and tied >= 1


# ---- matches and self-play ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", ["capture", "xiangqi"])
@pytest.mark.parametrize("sample_plies", [0, 2])
def test_match_on_wide_openings_equals_the_model(rules_golden, sample_plies, rules):
    """Match against match_model.play_match on 10 openings of 65-101 moves, both players "posabs" with more playouts than the widest
    root has children, 3 plies per game: wave_choose_prologue and k_match_choose over both rounds; rules "xiangqi" compacts the
    king-safe candidates over both rounds.  Condition (on the model): a chosen candidate of rank >= 64 — greedy with sample_plies 0,
    sampled with sample_plies 2."""
    from cchess_zero_amd.arena import Match
    t0 = time.time()
    op, want, ranks, sampled = W.match_reference(rules_golden, sample_plies, rules)
    hi = ranks >= 64
    assert (hi & sampled).sum() >= 1 if sample_plies else (hi & ~sampled).sum() >= 1
    players = [(MM.device_forward(m, s), p) for m, s, p in W.MATCH_PLAYERS]
    for slots in (2 * W.MATCH_OPENINGS, 6):
        res = Match(*players, op, slots=slots, max_plies=W.MATCH_PLIES, sample_plies=sample_plies, seed=W.MATCH_SEED, nodes_per_tree=1 << 15,
                    rules=rules).play()
        MM.assert_equals_model(res, want, (rules, sample_plies, slots))
    print("match, rules %s, sample_plies %d: %d choices of rank >= 64 greedy, %d sampled; %.1f s"
          % (rules, sample_plies, (hi & ~sampled).sum(), (hi & sampled).sum(), time.time() - t0))


def test_selfplay_choose_at_the_king_safe_level_equals_the_model(rules_golden):
    """k_sp_choose under rules "xiangqi" (no repetition rule) against selfplay_rules_model.play_games on 10 roots of 65-101 moves:
    pi, the Dirichlet noise and the pick over the king-safe root children alone, gamma[j] belonging to compacted child j; the
    packed records byte for byte.  Condition (on the model): a pick of rank >= 64 among the king-safe candidates."""
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    t0 = time.time()
    (boards, side, rr), want, ranks = W.selfplay_reference(rules_golden)
    assert (ranks >= 64).sum() >= 1 and want["min_margin"] >= 1e-12 and want["unsafe_plies"] >= 1
    eng = SearchEngine(len(boards), 1 << 15)
    sp = SelfPlay(eng, None, W.SP_PLAYOUTS, exploration=True, temperature=1.0, continuous=False, max_plies=W.SP_MAX_PLIES, rules="xiangqi",
                  repetition=0)
    sp.start(boards, side, rr)
    fwd = MM.device_forward(*W.NETS["posabs"])
    for rand in W.selfplay_stream(len(boards)):
        sp.step_ply(fwd, rand=rand)
    rec, st = sp.drain(), sp.stats()
    keys = ("games", "red_wins", "black_wins", "draws", "plies", "stalled", "mates", "repetitions", "perpetuals")
    assert {k: st[k] for k in keys} == {k: want["stats"][k] for k in keys} and st["dropped"] == 0
    assert np.array_equal(sp.active().numpy().astype(bool), want["active"])
    assert rec.shape == want["records"].shape and np.array_equal(rec, want["records"])
    print("self-play at the king-safe level: %s, %d picks of rank >= 64; %.1f s" % (want["stats"], (ranks >= 64).sum(), time.time() - t0))


# ---- the unmodified reference -------------------------------------------------------------------------------------------------------
class _HipK1:
    """searchdrive's interface over cz_search_select_k / cz_search_expand_backup_k with k = 1."""

    def __init__(self, G):
        from cchess_zero_amd.engine import SearchEngine
        self.e = SearchEngine(G, 200000)

    def reset(self, b, s, rr):
        self.e.reset(b, s, rr)

    def select(self, mode, mask=None):
        from cchess_zero_amd import _lib
        act = None if mask is None else torch.from_numpy(mask.astype(np.uint8)).cuda()
        self.e.ctx.call("cz_search_select_k", int(mode), 1, act, self.e.planes, _lib.F32, 14, self.e.need)
        return _np(self.e.planes), _np(self.e.need)

    def expand_backup(self, logits, value):
        from cchess_zero_amd import _lib
        self.e.ctx.call("cz_search_expand_backup_k", 1, torch.from_numpy(logits).cuda(), torch.from_numpy(value).cuda().contiguous(), _lib.F32)

    def root_stats(self):
        return self.e.root_stats_host()

    def advance(self, played):
        self.e.advance(played)

    def tree_dump(self, g):
        return self.e.tree_dump(g)

    def status(self):
        return _np(self.e.status()[0])


@pytest.mark.parametrize("path", ["width1", "k1"])
def test_search_matches_reference_on_wide_nodes(golden_dir, path):
    """The device search against the UNMODIFIED reference from open boards of 72-101 moves (tests/golden/mcts_wide.json: root
    children, whole-tree digests, evaluated positions; selected children up to index 100 under a root and 98 under another node),
    through k_select / k_expand_backup and through the k-wide kernels with k = 1."""
    from test_hip_search import _HipEngine
    cases = json.load(open(os.path.join(golden_dir, "mcts_wide.json")))["cases"]
    eng = _HipEngine(len(cases)) if path == "width1" else _HipK1(len(cases))
    results, logs = searchdrive.run_cases(eng, cases)
    assert not np.any(eng.status() & ~8)
    searchdrive.check_against_golden(results, logs, cases)
