"""The inputs of test_search_edges_gpu.py, checked on the C oracle alone: they DO drive the search onto the paths the GPU tests are
about (pool exhaustion at many different steps and in the middle of a k-wide step, CZ_ST_NO_MOVES, CZ_ST_MOVE_OVERFLOW), so the
inputs cannot drift into exercising nothing.  Runs anywhere."""
import numpy as np
import pytest

import search_edges as E
from oracle import oracle as O


def test_boards_are_what_the_status_paths_need():
    stuck, adv = E.stuck_board(), E.advisor_board()
    assert len(O.legal_moves(stuck, 0)) == 0 and len(O.legal_moves(stuck, 1)) == 2   # no moves, and not an overflow
    with pytest.raises(RuntimeError):
        O.legal_moves(adv, 0)
    assert len(O.legal_moves(adv, 1)) == 44


def test_corpus_slice(rules_golden):
    boards, side, rr = E.corpus_slice(rules_golden)
    counts = [len(O.legal_moves(boards[g], int(side[g]))) for g in range(len(boards))]
    assert len(boards) == 48 and min(counts) == 26 and max(counts) == 55
    assert rr.min() >= 0 and rr.max() <= 60 and np.all(rr[::5] == 57)


@pytest.mark.parametrize("K,cap,steps,mode", E.SMALL_POOLS)
def test_small_pools_exhaust_on_the_oracle(rules_golden, K, cap, steps, mode):
    """czo_search_expand_backup / _k with bf16-valued logits: at least 40 of the 48 trees fill their pool, at 4 or more different
    steps, for K > 1 at least 10 of them in a step in which another slot of the same tree still expanded; no tree picks up another
    status; no virtual loss stays in any tree and the exhausting simulation is counted."""
    boards, side, rr = E.corpus_slice(rules_golden)
    G = len(boards)
    orc = E.OracleSearch(G, cap, K)
    orc.reset(boards, side, rr)
    trace = E.lockstep(orc, steps, E.make_net(mode, E.SMALL_POOL_SALT, bf16=True))
    exhausted, at_steps, mixed, other = E.exhaustion_profile(trace)
    print("K=%d cap=%d: %d of %d trees exhaust, at steps %s, %d in a step that still expanded another slot" % (K, cap, exhausted, G, at_steps, mixed))
    assert exhausted >= 40 and len(at_steps) >= 4 and other == 0
    assert mixed >= 10 if K > 1 else mixed == 0
    st, nodes, sims = orc.status()
    assert np.all(nodes <= cap)
    leaves = 0
    for g in range(G):
        rec = orc.tree_dump(g)
        E.check_tree(rec, sims[g])
        E.check_resumed_tree(rec)
        # check_resumed_tree does notice a visit too many: claim one for an expanded node that has none
        p = next((p for p, r in E._paths(rec) if int(r[6]) > 0), None)
        if p is not None:
            with pytest.raises(AssertionError):
                E.check_resumed_tree(rec, {p: 1})
        leaves += len(E.visited_unexpanded(rec))
    assert leaves >= exhausted   # every exhausting simulation left its visit on a leaf without children


@pytest.mark.parametrize("K", [1, 4])
def test_status_quartet_on_the_oracle(K):
    """czo_search_select (`child_count == 0`, `n < 0`) and czo_search_select_k (both abandon branches): final status [2, 2, 4, 4];
    tree 1 completes 5 simulations before it selects the childless node; tree 3 keeps its 44 root children with N = 0 — the
    virtual loss taken back and the claimed node given back."""
    boards, side, rr, final = E.status_quartet()
    orc = E.OracleSearch(4, 4096, K)
    orc.reset(boards, side, rr)
    trace = E.lockstep(orc, E.QUARTET_STEPS, E.make_net(*E.QUARTET_NET))
    st, nodes, sims = orc.status()
    assert np.array_equal(st, final)
    assert np.array_equal(trace[-2]["status"], final), "reached before the last step: the last one runs on parked trees"
    assert sims[1] == 5 and sims[0] == 0 and sims[2] == 0 and sims[3] == 0
    rec = orc.tree_dump(3)
    assert len(rec) == 44 and not rec[:, 2].any() and np.all(rec[:, 6] == -1)
    assert len(orc.tree_dump(0)) == 0 and len(orc.tree_dump(2)) == 0
    for g in range(4):
        E.check_tree(orc.tree_dump(g), sims[g])
