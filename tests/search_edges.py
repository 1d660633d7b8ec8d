"""Shared pieces of test_search_edges_cpu.py / test_search_edges_gpu.py: inputs that drive the lock-step search (cz_search.hip) and
its C oracle onto their status paths — pool exhaustion, CZ_ST_NO_MOVES, CZ_ST_MOVE_OVERFLOW — the conditions that prove the inputs
do so (evaluated on the oracle alone), and a lock-step driver that a HIP engine can follow step by step."""
import numpy as np

import fakenet
from oracle import oracle as O
from test_scale_properties import _tree_invariants
from test_width import _OracleK, _budget_search_oracle   # noqa: F401 (the GPU tests take them from here)

ST_POOL_EXHAUSTED, ST_NO_MOVES, ST_MOVE_OVERFLOW, ST_BAD_ADVANCE = 1, 2, 4, 8   # include/cchess_hip.h: CZ_ST_*

# (K, nodes per tree, lock-steps, fakenet mode): pools so small that nearly every tree fills its own, at several different steps
SMALL_POOLS = [(1, 300, 30, "pos"), (4, 400, 24, "signed"), (16, 900, 16, "pos")]
SMALL_POOL_SALT = 77


def corpus_slice(g, n=48):
    """n corpus positions (both kings, at least one move) with restrict_round counters up to 60, every fifth at 57 (draws at depth 3)."""
    ok = [(g["boards"][i] == 1).any() and (g["boards"][i] == 8).any() and g["counts"][i] > 0 for i in range(len(g["boards"]))]
    idx = np.nonzero(ok)[0][::53][:n]
    rr = (np.arange(len(idx)) * 7 % 61).astype(np.int32)
    rr[::5] = 57
    return g["boards"][idx].copy(), g["side"][idx].copy(), rr


def stuck_board():
    """Red (K e2 behind P e1 and between A d2 / A f2) has no move at all and it is no overflow; black (k d9) has two."""
    b = np.zeros(90, np.uint8)
    b[13], b[21], b[22], b[23], b[84] = 6, 2, 1, 2, 8
    return b


def advisor_board():
    """The start position with red's advisor on e2, where no label exists for its moves: red's move list cannot be expressed
    (CZ_ST_MOVE_OVERFLOW), black has its 44 opening moves."""
    b = O.fen_to_board(O.START_FEN).copy()
    b[3], b[22] = 0, 2
    return b


def status_quartet():
    """-> boards [4, 90], side [4], rr [4], final status [4]: a root without moves, a root two plies above one, a root whose move
    list overflows, a root whose every child's does."""
    s, a = stuck_board(), advisor_board()
    return (np.stack([s, s, a, a]), np.array([0, 1, 0, 1], np.uint8), np.zeros(4, np.int32),
            np.array([ST_NO_MOVES, ST_NO_MOVES, ST_MOVE_OVERFLOW, ST_MOVE_OVERFLOW], np.int32))


QUARTET_STEPS, QUARTET_NET = 8, ("pos", 3)


def bf16_round(a):
    """float32 array -> the nearest bfloat16 values, as float32 (torch's round trip: what a bf16 net hands the search)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def make_net(mode, salt, bf16=False):
    """fakenet.make_forward; bf16: logits and value rounded to bfloat16, so that a float32 and a bf16 copy hold the same numbers."""
    fwd = fakenet.make_forward(mode, salt)
    if not bf16:
        return fwd

    def rounded(planes):
        lg, v = fwd(planes)
        return bf16_round(lg), bf16_round(v)
    return rounded


class OracleSearch:
    """O.Search behind one interface for both widths: K = 1 is the one-simulation-per-tree schedule (czo_search_select), K > 1 the
    k-wide one (czo_search_select_k)."""

    def __init__(self, G, cap, K):
        self.s, self.K, self.G = O.Search(G, cap), int(K), G

    def reset(self, boards, side, rr):
        self.s.reset(boards, side, rr)

    def select(self, mode, k=None):
        k = self.K if k is None else k
        self._k = k
        return self.s.select(mode) if self.K == 1 else self.s.select_k(mode, k)

    def expand_backup(self, logits, value):
        if self.K == 1:
            self.s.expand_backup(logits, value)
        else:
            self.s.expand_backup_k(self._k, logits, value)

    def __getattr__(self, name):    # status, root_stats, root_state, advance, tree_dump
        return getattr(self.s, name)


class MaskedOracleK(_OracleK):
    """_OracleK at width K: one czo_search per tree, so that a masked tree is simply not called."""

    def select(self, mode, mask=None):
        K = self.K
        planes = np.zeros((self.G * K, 9, 10, 14), np.float32)
        need = np.zeros(self.G * K, np.uint8)
        self._ran = np.zeros(self.G, bool)
        for g in range(self.G):
            if mask is not None and not mask[g]:
                continue
            planes[g * K:(g + 1) * K], need[g * K:(g + 1) * K] = self.e[g].select_k(mode, K)
            self._ran[g] = True
        return planes, need

    def expand_backup(self, logits, value):
        K = self.K
        for g in range(self.G):
            if self._ran[g]:
                self.e[g].expand_backup_k(K, logits[g * K:(g + 1) * K], value[g * K:(g + 1) * K])

    def status(self):
        st = [e.status() for e in self.e]
        return tuple(np.concatenate([s[i] for s in st]) for i in range(3))


def lockstep(orc, steps, net, follower=None, select_args=None, start=0):
    """Lock-steps start .. start + steps - 1 of `orc` (step 0 is the mode-0 one); a `follower` (the HIP engine under test) sees each:
    follower.select(step, mode, planes, need, **args) right after the oracle's select, with the oracle's rows to compare its own with,
    follower.expand_backup(step, logits, value) with the very numbers the oracle gets, follower.after(step) behind both.
    select_args(step) -> keyword arguments of both selects (mask=, k=).  -> per step dict(status, nodes, sims) after the step."""
    trace = []
    for step in range(start, start + steps):
        mode = 0 if step == 0 else 1
        args = select_args(step) if select_args else {}
        planes, need = orc.select(mode, **args)
        if follower is not None:
            follower.select(step, mode, planes, need, **args)
        logits, value = net(planes)
        orc.expand_backup(logits, value)
        if follower is not None:
            follower.expand_backup(step, logits, value)
            follower.after(step)
        st, nodes, sims = orc.status()
        trace.append(dict(status=st.copy(), nodes=nodes.copy(), sims=sims.copy()))
    return trace


def exhaustion_profile(trace):
    """-> (trees that exhausted their pool, the steps at which one did, trees that did so in a step in which another of their slots
    still expanded — their node count grew in that very step —, union of all other status bits)."""
    G = len(trace[0]["status"])
    prev_st, prev_nodes = np.zeros(G, np.int32), np.ones(G, np.int32)
    steps, mixed = set(), np.zeros(G, bool)
    for step, t in enumerate(trace):
        newly = ((t["status"] & ST_POOL_EXHAUSTED) != 0) & ((prev_st & ST_POOL_EXHAUSTED) == 0)
        if newly.any():
            steps.add(step)
        mixed |= newly & (t["nodes"] > prev_nodes)
        prev_st, prev_nodes = t["status"], t["nodes"]
    last = trace[-1]["status"]
    return int(((last & ST_POOL_EXHAUSTED) != 0).sum()), sorted(steps), int(mixed.sum()), int(np.bitwise_or.reduce(last & ~ST_POOL_EXHAUSTED))


def check_tree(rec, sims=None):
    """_tree_invariants (no virtual loss left in the tree: N = 1 + sum of the children's, Q = W / N) and, with `sims`, every
    completed simulation counted in exactly one root child."""
    _tree_invariants(rec)
    if sims is not None:
        assert int(sum(int(r[2]) for r in rec if int(r[0]) == 0)) == int(sims)


def _paths(rec):
    """The records of a pre-order dump with the move labels from the root down to each, as a tuple: a node's name across dumps."""
    path = []
    for r in rec:
        del path[int(r[0]):]
        path.append(int(r[1]))
        yield tuple(path), r


def visited_unexpanded(rec):
    """{path: N} of the visited records without children: king captures and 60-ply draws, which stay that way — and the leaves whose
    expansion found the pool full.  Their simulation was backed up and counted all the same (the `!fits` branches), so such a leaf
    carries a visit that expanded nothing; when the tree goes on behind cz_search_advance it is evaluated again and expanded then."""
    return {p: int(r[2]) for p, r in _paths(rec) if int(r[2]) > 0 and int(r[6]) == -1}


def check_resumed_tree(rec, carried=None):
    """_tree_invariants for a tree that went on after a full pool: every expanded, visited node has Q == W / N in float32, |Q| <= 1 and
    N == 1 + sum(children N) + carried.get(path, 0), where `carried` is visited_unexpanded() of the dump taken when the tree resumed —
    exactly the visits that expanded nothing, at exactly those nodes.  With nothing carried this IS _tree_invariants."""
    carried = carried or {}
    if not carried:
        _tree_invariants(rec)
    child_sum = {}
    for p, r in _paths(rec):
        child_sum[p[:-1]] = child_sum.get(p[:-1], 0) + int(r[2])
    for p, r in _paths(rec):
        N, nc = int(r[2]), int(r[6])
        if N > 0:
            W, Q = np.int32(r[3]).view(np.float32), np.int32(r[4]).view(np.float32)
            assert Q == np.float32(W / np.float32(N)) or (np.isnan(Q) and np.isnan(W)), p
            assert abs(float(Q)) <= 1.0 + 1e-6, p
        if nc > 0:
            assert N == 1 + child_sum.get(p, 0) + carried.get(p, 0), (p, N, child_sum.get(p, 0), carried.get(p, 0))


def most_visited(stats):
    """The most visited root child of every tree, first maximum; 0xFFFF where the root has none."""
    G = len(stats["count"])
    played = np.full(G, 0xFFFF, np.uint16)
    for t in range(G):
        n = int(stats["count"][t])
        if n:
            played[t] = stats["label"][t, int(np.argmax(stats["N"][t, :n]))]
    return played
