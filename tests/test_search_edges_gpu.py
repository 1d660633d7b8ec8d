"""The status paths and the k-wide variants of the lock-step search (cz_search.hip) against the C oracle, bit for bit: no tolerance
anywhere, floats are compared as their bits.  test_search_edges_cpu.py proves on the oracle alone that the inputs reach the paths.

Exercised here and nowhere else in the suite:
  * the `!fits` branches of k_expand_backup and k_expand_backup_k (pool exhaustion: trees, counters and the exhausting
    simulation's backup; at width k the claimed leaf is given back, child_begin = -1, and its virtual loss unwound);
  * cz_search_advance clearing CZ_ST_POOL_EXHAUSTED, and the tree going on in the room the compaction made;
  * k_select_k<uint16_t>, k_expand_backup_k<uint16_t> and bf16 logits into k_expand_backup<uint16_t, false>;
  * `cc == 0` (CZ_ST_NO_MOVES) and `nmoves < 0` (CZ_ST_MOVE_OVERFLOW) in select_body, both abandon branches of k_select_k
    (take_back_vl; on overflow the claimed node given back as well);
  * a parked row under k_select_k (the active mask at width k), and rows of trees that do not descend: write_leaf(zero = true)
    must overwrite what the buffers held — every select here starts from planes full of ones and needs_eval full of 0xFF;
  * the slot stride g * k + j of select(k=...) with k below the engine's width and more than one tree."""
import numpy as np
import pytest
import torch

import search_edges as E

pytestmark = pytest.mark.gpu

MAXREC = 1 << 16   # tree_dump records: far above the largest tree here


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _status(eng):
    return tuple(_np(x) for x in eng.status()[:3])


class _Follower:
    """The HIP engine behind search_edges.lockstep: every select starts from stale buffers and is compared with the oracle's rows."""

    def __init__(self, eng, orc=None, bf16_inputs=False, per_step=False):
        self.eng, self.orc, self.per_step = eng, orc, per_step
        self.in_dtype = torch.bfloat16 if bf16_inputs else torch.float32

    def select(self, step, mode, oplanes, oneed, mask=None, k=None):
        eng = self.eng
        eng.planes.fill_(1)
        eng.need.fill_(0xFF)
        hp, hn = eng.select(mode, active=None if mask is None else mask.astype(np.uint8), k=k)
        rows = len(oneed)
        assert hp.shape[0] == rows and hn.shape[0] == rows
        assert np.array_equal(_np(hn), oneed), step
        hp = hp.float()
        # every row, also those of parked, stopped and masked trees: the oracle's planes (zeros without a leaf), +0 in the channels beyond
        assert np.array_equal(_bits(_np(hp[..., :14])), _bits(oplanes)), step
        assert not bool(hp[..., 14:].any()), step
        # rows behind the G * k of this call belong to nobody: untouched
        assert bool((eng.planes[rows:] == 1).all()) and bool((eng.need[rows:] == 0xFF).all()), step

    def expand_backup(self, step, logits, value):
        dev = self.eng.dev
        self.eng.expand_backup(torch.from_numpy(logits).to(dev).to(self.in_dtype), torch.from_numpy(value).to(dev).to(self.in_dtype))

    def after(self, step):
        if self.per_step:
            hst, _, hsims = _status(self.eng)
            ost, _, osims = self.orc.status()
            assert np.array_equal(hst, ost) and np.array_equal(hsims, osims), step


def _same_root_stats(eng, orc):
    hs, os_ = eng.root_stats_host(), orc.root_stats()
    for key in ("label", "N", "count"):
        assert np.array_equal(hs[key], os_[key]), key
    for key in ("Q", "P", "W"):
        assert np.array_equal(_bits(hs[key]), _bits(os_[key])), key
    return os_


def _same_trees(eng, orc, G, sims=None):
    for g in range(G):
        rec = eng.tree_dump(g, MAXREC)
        assert np.array_equal(rec, orc.tree_dump(g)), g
        E.check_tree(rec, None if sims is None else sims[g])


def _same_search(eng, orc, G, nodes_too=True):
    """status, simulation counters, root statistics and every whole tree equal the oracle's; no virtual loss left anywhere and
    every counted simulation in exactly one root child.  -> (oracle root stats, status)"""
    hst, hnodes, hsims = _status(eng)
    ost, onodes, osims = orc.status()
    assert np.array_equal(hst, ost) and np.array_equal(hsims, osims)
    if nodes_too:
        assert np.array_equal(hnodes, onodes)
    stats = _same_root_stats(eng, orc)
    _same_trees(eng, orc, G, hsims)
    return stats, hst


# K = 1 takes all three plane formats, K = 4 float32 and bf16, K = 16 fp16: every width sees a 16-bit format, K = 1 bf16 logits
_POOL_CASES = [E.SMALL_POOLS[0] + (torch.float32, 14), E.SMALL_POOLS[0] + (torch.bfloat16, 16), E.SMALL_POOLS[0] + (torch.float16, 16),
               E.SMALL_POOLS[1] + (torch.float32, 14), E.SMALL_POOLS[1] + (torch.bfloat16, 16), E.SMALL_POOLS[2] + (torch.float16, 16)]


@pytest.mark.parametrize("K,cap,steps,mode,plane_dtype,channels", _POOL_CASES, ids=["K1-f32", "K1-bf16", "K1-f16", "K4-f32", "K4-bf16", "K16-f16"])
def test_pool_exhaustion_equals_oracle_and_advance_resumes(rules_golden, K, cap, steps, mode, plane_dtype, channels):
    """The `!fits` branches of k_expand_backup (K = 1) and k_expand_backup_k (K = 4, 16): 46 or 47 of 48 trees fill their pool, at
    seven or eight different steps, most k-wide ones while another slot of the same step still expands.  With 16-bit planes the
    logits and values arrive as bf16 — k_expand_backup<uint16_t, false> at K = 1, k_select_k<uint16_t> / k_expand_backup_k<uint16_t>
    at K > 1 — and hold the very numbers the oracle gets as float32.  Then cz_search_advance: CZ_ST_POOL_EXHAUSTED cleared, the
    kept subtree the oracle's, and the trees search on in the room the compaction made.
    (What no test can see through the API: whether the `!fits` branch of k_expand_backup_k puts child_begin[leaf] back from
    "pending" to "unexpanded".  The tree is parked from then on, tree_dump and cz_search_lines read either as "no children", and
    advance_tree, the only way back, rewrites every negative record to -1.  Its unwinding of the path IS seen: the invariants.)"""
    from cchess_zero_amd.engine import SearchEngine
    boards, side, rr = E.corpus_slice(rules_golden)
    G = len(boards)
    eng = SearchEngine(G, cap, plane_dtype=plane_dtype, channels=channels, width=K)
    orc = E.OracleSearch(G, cap, K)
    eng.reset(boards, side, rr)
    orc.reset(boards, side, rr)
    sixteen = plane_dtype != torch.float32
    trace = E.lockstep(orc, steps, E.make_net(mode, E.SMALL_POOL_SALT, bf16=True), _Follower(eng, orc, bf16_inputs=sixteen))
    exhausted, at_steps, mixed, other = E.exhaustion_profile(trace)
    assert exhausted >= 40 and len(at_steps) >= 4 and other == 0 and (mixed >= 10 if K > 1 else True)
    stats, status = _same_search(eng, orc, G)
    # ---- re-root at the most visited child
    played = E.most_visited(stats)
    moved = played != 0xFFFF
    assert moved.all()
    eng.advance(played)
    orc.advance(played)
    hst, hnodes, hsims = _status(eng)
    assert np.array_equal(hst[moved], status[moved] & ~E.ST_POOL_EXHAUSTED) and not hsims[moved].any()
    for h, o in zip(eng.root_state(), orc.root_state()):
        assert np.array_equal(_np(h), o)
    carried = []
    for g in range(G):
        rec = eng.tree_dump(g, MAXREC)
        assert np.array_equal(rec, orc.tree_dump(g)), g
        carried.append(E.visited_unexpanded(rec))
        assert hnodes[g] == len(rec) + 1, g     # advance_tree compacts: the pool holds the kept subtree, its root included, and nothing else
    # ---- the HIP engine alone (the oracle does not compact: it is no reference past this point), float32 inputs from its own planes
    fwd = E.make_net(mode, E.SMALL_POOL_SALT)
    grown = 0
    for step in range(4):
        _, before, _ = _status(eng)
        planes, need = eng.select(1)
        lg, v = fwd(_np(planes.float()[..., :14]))
        eng.expand_backup(torch.from_numpy(lg).to(eng.dev), torch.from_numpy(v).to(eng.dev))
        _, after, _ = _status(eng)
        # a tree that asks for an evaluation with room for a whole move list (128) left must grow by that expansion; the others
        # (a leaf that is a king capture or a 60-ply draw needs no net) may not have to
        must = _np(need).reshape(G, K).any(axis=1) & (before + 128 <= cap)
        assert np.all(after[must] > before[must]), step
        assert np.all(after >= before) and np.all(after <= cap)
        grown += int(must.sum())
    assert grown > 0
    st, nodes, sims = _status(eng)
    live = ((hst & ~E.ST_BAD_ADVANCE) == 0) & ((st & (E.ST_NO_MOVES | E.ST_MOVE_OVERFLOW)) == 0)
    assert live.any() and np.all(sims[live] > 0)
    # _tree_invariants as it stands cannot hold here, and not because of a fault: the simulation that found the pool full was backed up
    # and counted without expanding its leaf (both kernels and the oracle say so), so the leaf carries one visit that expanded nothing
    # and is evaluated once more when the tree goes on.  check_resumed_tree asks for N == 1 + sum(children N) + exactly that visit at
    # exactly those leaves, and for plain _tree_invariants on every tree that carried none.
    for g in range(G):
        E.check_resumed_tree(eng.tree_dump(g, MAXREC), carried[g])


@pytest.mark.parametrize("K", [1, 4])
def test_status_quartet_equals_oracle(K):
    """CZ_ST_NO_MOVES and CZ_ST_MOVE_OVERFLOW inside the search.  K = 1: `cc == 0` and `nmoves < 0` in select_body (k_select; then
    again with terminal simulations completing inside the launch, and through k_select_cache).  K = 4: both abandon branches of
    k_select_k — take_back_vl on a childless node; on a move list that cannot be expressed the claimed node given back as well, so
    that tree 3 keeps 44 root children with N = 0.  need, planes (also the rows of the trees that have stopped), status and sims
    every step, whole trees at the end; final status [2, 2, 4, 4]."""
    from cchess_zero_amd.engine import SearchEngine
    boards, side, rr, final = E.status_quartet()
    net = E.make_net(*E.QUARTET_NET)
    eng = SearchEngine(4, 4096, width=K)
    orc = E.OracleSearch(4, 4096, K)
    eng.reset(boards, side, rr)
    orc.reset(boards, side, rr)
    E.lockstep(orc, E.QUARTET_STEPS, net, _Follower(eng, orc, per_step=True))
    _, status = _same_search(eng, orc, 4)
    assert np.array_equal(status, final)
    rec = eng.tree_dump(3, MAXREC)
    assert len(rec) == 44 and not rec[:, 2].any() and np.all(rec[:, 6] == -1)
    if K != 1:
        return
    for variant in ("terminal_extra", "eval_cache"):
        e2 = SearchEngine(4, 4096)
        try:
            if variant == "eval_cache":
                e2.set_eval_cache(True)
            else:
                e2.set_terminal_extra(4)
            e2.reset(boards, side, rr)
            for step in range(E.QUARTET_STEPS):
                parked = torch.from_numpy((_status(e2)[0] & ~E.ST_BAD_ADVANCE) != 0).to(e2.dev)
                e2.planes.fill_(1)
                e2.need.fill_(0xFF)
                planes, need = e2.select(0 if step == 0 else 1)
                assert not bool(planes[parked].any()) and not bool(need[parked].any()), (variant, step)
                lg, v = net(_np(planes))
                e2.expand_backup(torch.from_numpy(lg).to(e2.dev), torch.from_numpy(v).to(e2.dev))
            # the same trees after the same simulations: a tree's simulations are sequential, whatever a launch completes of them
            _, status = _same_search(e2, orc, 4)
            assert np.array_equal(status, final), variant
        finally:
            if variant == "eval_cache":
                e2.set_eval_cache(False)
            else:
                e2.set_terminal_extra(0)


def test_active_mask_at_width_k_equals_oracle(rules_golden):
    """A parked row under k_select_k: K = 4, 24 trees, from step 1 on tree g sits out the steps with (g + step) % 3 == 0.  The
    reference is one oracle search per tree, not called for a masked tree.  A masked tree's K rows are zero planes with
    needs_eval = 0 (over stale buffers) and its tree and counters do not change.  Then SearchEngine.search(active = mask), what
    Analyzer.analyse runs: parked trees stay empty, the others equal the oracle's budgeted search of those trees alone."""
    from cchess_zero_amd.engine import SearchEngine
    boards, side, rr = E.corpus_slice(rules_golden, 24)
    G, K, cap = len(boards), 4, 60000
    eng = SearchEngine(G, cap, width=K)
    orc = E.MaskedOracleK(G, K, cap)
    eng.reset(boards, side, rr)
    orc.reset(boards, side, rr)

    def mask_of(step):
        return np.ones(G, bool) if step == 0 else (np.arange(G) + step) % 3 != 0

    class Follower(_Follower):
        def select(self, step, mode, oplanes, oneed, mask=None, k=None):
            self.masked = np.nonzero(~mask)[0]
            self.before = (_status(self.eng)[2], [self.eng.tree_dump(int(g), MAXREC) for g in self.masked])
            super().select(step, mode, oplanes, oneed, mask=mask)
            assert not oneed.reshape(G, K)[self.masked].any()

        def after(self, step):
            super().after(step)
            sims = _status(self.eng)[2]
            assert np.array_equal(sims[self.masked], self.before[0][self.masked]), step
            for g, rec in zip(self.masked, self.before[1]):
                assert np.array_equal(self.eng.tree_dump(int(g), MAXREC), rec), (step, g)

    E.lockstep(orc, 12, E.make_net("signed", 77), Follower(eng, orc, per_step=True), select_args=lambda step: dict(mask=mask_of(step)))
    _same_search(eng, orc, G)
    # ---- SearchEngine.search with a fixed mask, on a fresh engine
    playouts = 40
    fk = E.make_net("pos", 9)

    def fwd_dev(planes):
        lg, v = fk(_np(planes.float()))
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    mask = np.arange(G) % 3 != 0
    act = np.nonzero(mask)[0]
    eng = SearchEngine(G, cap, width=K)
    eng.reset(boards, side, rr)
    steps = eng.search(fwd_dev, playouts, active=mask.astype(np.uint8))
    sub = E.O.Search(len(act), cap)
    sub.reset(boards[act], side[act], rr[act])
    assert steps == E._budget_search_oracle(sub, fk, K, playouts)
    hst, hnodes, hsims = _status(eng)
    ost, onodes, osims = sub.status()
    assert np.all(hsims[act] == playouts) and np.array_equal(hsims[act], osims) and np.array_equal(hst[act], ost)
    assert np.array_equal(hnodes[act], onodes)
    assert not hsims[~mask].any() and not hst[~mask].any() and np.all(hnodes[~mask] == 1)
    hs, os_ = eng.root_stats_host(), sub.root_stats()
    assert np.array_equal(hs["N"][act], os_["N"]) and np.array_equal(_bits(hs["Q"][act]), _bits(os_["Q"]))
    assert not hs["count"][~mask].any()
    for i, g in enumerate(act):
        rec = eng.tree_dump(int(g), MAXREC)
        assert np.array_equal(rec, sub.tree_dump(i)), g
        E.check_tree(rec, playouts)
    for g in np.nonzero(~mask)[0]:
        assert len(eng.tree_dump(int(g), MAXREC)) == 0, g


def test_k_below_the_engines_width_equals_oracle(rules_golden):
    """select(k = 4) on an engine of width 16, as main.py's MCTS_tree drives it, with FIVE trees: the pending slots and the net's
    rows are strided g * k + j, not g * width + j, and the rows behind G * k stay untouched.  Then k = 16 on the same engine and
    the same oracle: the smaller k has left no pending state behind."""
    from cchess_zero_amd.engine import SearchEngine
    boards, side, rr = E.corpus_slice(rules_golden, 5)
    G, W, cap = len(boards), 16, 60000
    eng = SearchEngine(G, cap, width=W)
    orc = E.OracleSearch(G, cap, W)
    eng.reset(boards, side, rr)
    orc.reset(boards, side, rr)
    net = E.make_net("signed", 77)
    fol = _Follower(eng, orc, per_step=True)
    E.lockstep(orc, 20, net, fol, select_args=lambda step: dict(k=4))
    _same_search(eng, orc, G)
    E.lockstep(orc, 5, net, fol, select_args=lambda step: dict(k=16), start=20)
    _same_search(eng, orc, G)
