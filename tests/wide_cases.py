"""Shared pieces of test_wide_nodes_cpu.py / test_wide_nodes_gpu.py (TEST INFRASTRUCTURE): roots with up to 101 children, the nets that
make a search select among children 64..127 — the second round of 64 lanes of every kernel that walks a node's children — and the
conditions that prove it, evaluated on the C oracle's root_stats and tree_dump alone.

Why two nets.  The root is never backed up (quirk Q2): its score is Q alone and it walks its children in index order until one
has a positive Q.  fakenet "signed" therefore never reaches a root child of index >= 64, but it does select such children inside
wide NON-root nodes; fakenet "posabs" (value |v|) gives every visited root child a negative Q, so the root walks its whole list."""
import functools

import numpy as np

import search_edges as E
from conftest import open_boards
from oracle import oracle as O

N_OPEN, SEED = 96, 41        # open_boards(96, 41): every third one climbs to ~100 moves
EVERY = 8                    # every 8th tree is a corpus position: a workgroup's neighbours are narrow
PLIES, PLAYOUTS = 3, 140     # per ply: the root step and 140 lock-steps, more than the widest root has children
NETS = {"signed": ("signed", 23), "posabs": ("posabs", 29)}   # name -> (fakenet mode, salt)
CAP = 60000


def roots(rules_golden):
    """-> boards [63, 90], side [63], rr [63], all with both kings and a move: the 32 climbers of open_boards(96, 41) (89-100+
    moves), its first 16 other boards (30-75 moves), the first 8 climbers once more with the OTHER side to move (a narrow root
    whose every child is a node of ~100 children, visited dozens of times), and in every 8th slot a corpus position;
    restrict_round counters like search_edges.corpus_slice, every fifth at 57."""
    ob, os_ = open_boards(N_OPEN, SEED)
    climbers = list(range(2, N_OPEN, 3))
    others = [i for i in range(N_OPEN) if i % 3 != 2][:16]
    wide = [(ob[i], int(os_[i])) for i in climbers + others] + [(ob[i], 1 - int(os_[i])) for i in climbers[:8]]
    order = np.random.default_rng(SEED).permutation(len(wide))
    wide = [wide[int(i)] for i in order]
    cb, cs, _ = E.corpus_slice(rules_golden, len(wide) // (EVERY - 1))
    boards, side, k, c = [], [], 0, 0
    while k < len(wide):
        if len(boards) % EVERY == EVERY - 1:
            boards.append(cb[c]); side.append(int(cs[c])); c += 1
        else:
            boards.append(wide[k][0]); side.append(wide[k][1]); k += 1
    boards, side = np.stack(boards), np.array(side, np.uint8)
    assert all((b == 1).any() and (b == 8).any() and len(O.legal_moves(b, int(s))) > 0 for b, s in zip(boards, side))
    rr = (np.arange(len(boards)) * 7 % 61).astype(np.int32)
    rr[::5] = 57
    return boards, side, rr


def widths(boards, side):
    return np.array([len(O.legal_moves(boards[i], int(side[i]))) for i in range(len(boards))])


def net(name, bf16=False):
    mode, salt = NETS[name]
    return E.make_net(mode, salt, bf16=bf16)


def sibling_index(rec):
    """The index of every record of a pre-order dump among its parent's children: the count of earlier records of equal depth
    under the same parent."""
    rec = np.asarray(rec).reshape(-1, 7)
    out = np.zeros(len(rec), np.int64)
    nxt = []            # nxt[d] = the next sibling index at depth d under the current parent
    for k in range(len(rec)):
        d = int(rec[k, 0])
        del nxt[d + 1:]
        if len(nxt) <= d:
            nxt.append(0)
        out[k] = nxt[d]
        nxt[d] += 1
    return out


ZERO = dict(expanded_gt64=0, expanded_gt96=0, inner_sel_ge64=0, inner_sel_ge96=0, root_sel_ge64=0, root_sel_ge96=0, played_ge64=0)


def conditions(stats, dumps):
    """The condition counts of one ply over all trees, from the oracle's root_stats and tree dumps only:
      expanded_gt64 / gt96   expanded nodes (the root included) with more than 64 / 96 children
      inner_sel_ge64 / ge96  selected (N > 0) children of index >= 64 / 96 under non-root parents
      root_sel_ge64 / ge96   the same under the root
      played_ge64            trees whose most visited root child (first maximum) has index >= 64"""
    c = dict(ZERO)
    for g, rec in enumerate(dumps):
        rec = np.asarray(rec).reshape(-1, 7)
        n = int(stats["count"][g])
        kids = np.concatenate([[n], rec[:, 6]]) if len(rec) else np.array([n])
        c["expanded_gt64"] += int((kids > 64).sum())
        c["expanded_gt96"] += int((kids > 96).sum())
        if not len(rec):
            continue
        idx = sibling_index(rec)
        sel, inner = rec[:, 2] > 0, rec[:, 0] > 0
        c["inner_sel_ge64"] += int((sel & inner & (idx >= 64)).sum())
        c["inner_sel_ge96"] += int((sel & inner & (idx >= 96)).sum())
        c["root_sel_ge64"] += int((sel & ~inner & (idx >= 64)).sum())
        c["root_sel_ge96"] += int((sel & ~inner & (idx >= 96)).sum())
        if n and int(np.argmax(stats["N"][g, :n])) >= 64:
            c["played_ge64"] += 1
    return c


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def oracle_run(boards, side, rr, name, plies=PLIES, playouts=PLAYOUTS, bf16=False, K=1, keep_dumps=True):
    """The oracle's search of these roots: per ply dict(stats, dumps, status, played, cond, state) — the root step and `playouts`
    lock-steps (width K: `playouts` lock-steps of K slots), then the most visited child is played."""
    G = len(boards)
    orc = E.OracleSearch(G, CAP, K)
    orc.reset(boards, side, rr)
    fwd = net(name, bf16)
    out = []
    for ply in range(plies):
        E.lockstep(orc, playouts + 1, fwd)
        stats = orc.root_stats()
        dumps = [orc.tree_dump(g) for g in range(G)]
        played = E.most_visited(stats)
        cond = conditions(stats, dumps)
        status = tuple(x.copy() for x in orc.status())
        orc.advance(played)
        out.append(dict(stats=stats, dumps=dumps if keep_dumps else None, status=status, played=played, cond=cond,
                        state=tuple(x.copy() for x in orc.root_state())))
    return out


@functools.lru_cache(maxsize=None)
def _cached_run(name, bf16):
    return oracle_run(*_STATE["roots"], name, bf16=bf16)


_STATE = {}       # "roots", "golden": set once per process by reference_roots (rules.npz is one file: the roots never differ)


def reference(rules_golden, name, bf16=False):
    """(roots, oracle_run(*roots, name, bf16=bf16)), computed once per process and net; read-only."""
    return reference_roots(rules_golden), _cached_run(name, bf16)


# ---- width k: budgeted searches (SearchEngine.search's schedule, test_width._budget_search_oracle) -----------------------------
K_PLIES, K_CAP = 2, 60000


def oracle_run_k(boards, side, rr, name, K, plies=K_PLIES, playouts=PLAYOUTS):
    """Per ply: exactly `playouts` simulations per tree with K in flight (czo_search_select_k under set_sim_target), then the most
    visited child is played.  -> per ply dict(steps, stats, dumps, status, played, cond)."""
    G = len(boards)
    orc = O.Search(G, K_CAP)
    orc.reset(boards, side, rr)
    fwd = net(name)
    out = []
    for ply in range(plies):
        steps = E._budget_search_oracle(orc, fwd, K, playouts)
        stats = orc.root_stats()
        dumps = [orc.tree_dump(g) for g in range(G)]
        played = E.most_visited(stats)
        out.append(dict(steps=steps, stats=stats, dumps=dumps, status=tuple(x.copy() for x in orc.status()), played=played,
                        cond=conditions(stats, dumps)))
        orc.advance(played)
    return out


@functools.lru_cache(maxsize=None)
def _cached_run_k(name, K):
    return oracle_run_k(*_STATE["roots"], name, K)


def reference_k(rules_golden, name, K):
    return reference_roots(rules_golden), _cached_run_k(name, K)


def reference_roots(rules_golden):
    if "roots" not in _STATE:
        _STATE["roots"], _STATE["golden"] = roots(rules_golden), rules_golden
    return _STATE["roots"]


K4_STEPS = 48


def k4_mask(G, step):
    """The trees that take part in lock-step `step` of the K = 4 run with parked rows: all in step 0, then tree g sits out the
    steps with (g + step) % 3 == 0."""
    return np.ones(G, bool) if step == 0 else (np.arange(G) + step) % 3 != 0


def k4_masked_oracle(boards, side, rr):
    """One oracle search per tree (search_edges.MaskedOracleK), reset on the roots: the reference of the run with parked rows."""
    orc = E.MaskedOracleK(len(boards), 4, K_CAP)
    orc.reset(boards, side, rr)
    return orc


# ---- the policy FC inside the expansion -----------------------------------------------------------------------------------------
FC_TREES, FC_PLIES, FC_STEPS = 24, 2, 60


def fc_weights():
    rng = np.random.default_rng(7)
    return (rng.standard_normal((2086, 180)) * 0.3).astype(np.float32), (rng.standard_normal(2086) * 0.2).astype(np.float32)


def fc_net(planes):
    """A "net" whose head-conv outputs z [B, 90, 3] and value [B, 1] are deterministic functions of a row's leaf planes [B,9,10,14]
    (test_hip_search.test_expand_with_folded_policy_fc_vs_oracle's)."""
    B = planes.shape[0]
    feat = np.ascontiguousarray(planes, np.float32).reshape(B, -1)
    z = np.maximum(0, (feat[:, :270] * 0.7 + feat[:, 270:540] * 0.31 + feat[:, 540:810] * 0.05 - 0.2)).astype(np.float32).reshape(B, 90, 3)
    z = (z + (feat.sum(axis=1, keepdims=True) % 7).astype(np.float32)[:, :, None] * 0.01).astype(np.float32)
    value = np.tanh(feat[:, ::9].sum(axis=1, keepdims=True) * 0.01 - 1.0).astype(np.float32)
    return z, value


@functools.lru_cache(maxsize=None)
def _cached_fc():
    import searchdrive
    boards, side, rr = (x[:FC_TREES] for x in _STATE["roots"])
    w, b = fc_weights()
    orc = O.Search(FC_TREES, CAP)
    orc.reset(boards, side, rr)
    out = []
    for ply in range(FC_PLIES):
        rows = 0
        for step in range(FC_STEPS + 1):
            planes, need = orc.select(0 if step == 0 else 1)
            rows += int(need.sum())
            z, value = fc_net(planes)
            orc.expand_backup(searchdrive.fc_logits_restated(z, w, b), value)
        stats = orc.root_stats()
        dumps = [orc.tree_dump(g) for g in range(FC_TREES)]
        played = E.most_visited(stats)
        out.append(dict(stats=stats, dumps=dumps, status=tuple(x.copy() for x in orc.status()), played=played, cond=conditions(stats, dumps),
                        rows=rows))
        orc.advance(played)
    return out


def reference_fc(rules_golden):
    """The oracle fed the full logits of the FC restated in NumPy (searchdrive.fc_logits_restated) on the first 24 roots; rows: the
    leaves of the ply that needed the net."""
    r = reference_roots(rules_golden)
    return tuple(x[:FC_TREES] for x in r), _cached_fc()


# ---- the evaluation cache: transpositions inside one tree ----------------------------------------------------------------------
def transpositions(board, side, rec):
    """Over one tree's dump from the root (board, side): -> (D, W): the expanded nodes whose position (board and side to move)
    an earlier-listed expanded node of the tree has as well, and those of them with more than 64 children.  Every such node was
    expanded either from the net or from the cache's copy of the other; positions are the cache's identity (rr is not part)."""
    rec = np.asarray(rec).reshape(-1, 7)
    seen = {(np.asarray(board, np.uint8).tobytes(), int(side))}
    path = [(np.asarray(board, np.uint8), int(side))]
    D = Wd = 0
    for r in rec:
        d = int(r[0])
        del path[d + 1:]
        if int(r[6]) <= 0:
            continue
        b, s = path[d]
        nb = O.apply_move(b, int(r[1]))[0]
        path.append((nb, s ^ 1))
        key = (nb.tobytes(), s ^ 1)
        if key in seen:
            D += 1
            Wd += int(r[6]) > 64
        seen.add(key)
    return D, Wd


# ---- principal variations -------------------------------------------------------------------------------------------------------
def lines_conditions(stats, dumps):
    """-> (root children of index >= 64 with N > 0 — each starts a line of its own —, trees in which a child of index < 64 and one
    of index >= 64 have the same N > 0: the order of their lines is decided by the first-index rule across the two rounds, steps
    of a line BELOW the root into a most visited child of index >= 64)."""
    import lines_model as LM
    starts = ties = below = 0
    for g in range(len(stats["count"])):
        n = int(stats["count"][g])
        v = stats["N"][g, :n]
        starts += int((v[64:] > 0).sum())
        ties += int(len(set(v[:64][v[:64] > 0].tolist()) & set(v[64:][v[64:] > 0].tolist())) > 0)
        rec = np.asarray(dumps[g]).reshape(-1, 7)
        first, kids = LM.children_of(rec)
        for k in first:
            while rec[k, LM.COUNT] > 0 and kids[k]:
                b = LM.first_max([int(rec[c, LM.N]) for c in kids[k]])
                if rec[kids[k][b], LM.N] <= 0:
                    break
                below += b >= 64
                k = kids[k][b]
    return starts, ties, below


# ---- matches and self-play ------------------------------------------------------------------------------------------------------
MATCH_OPENINGS, MATCH_PLIES, MATCH_SEED = 10, 3, 5
MATCH_PLAYERS = (("posabs", 29, 120), ("posabs", 31, 110))      # (fakenet mode, salt, playouts): more playouts than any root has children
SP_TREES, SP_PLAYOUTS, SP_STEPS, SP_MAX_PLIES = 10, 120, 3, 2


def wide_subset(rules_golden, n):
    """The first n roots with more than 64 moves and no move that takes a king (the game goes on behind the first ply)."""
    boards, side, rr = reference_roots(rules_golden)
    pick = []
    for i in range(len(boards)):
        mv = O.legal_moves(boards[i], int(side[i]))
        if len(mv) > 64 and all(O.apply_move(boards[i], int(a))[2] == 0 for a in mv):
            pick.append(i)
    assert len(pick) >= n
    pick = pick[:n]
    return boards[pick], side[pick], rr[pick]


class _Ranks:
    """Wraps a model's choice function (-> index among the candidates it was given, or a tuple that starts with it): records the
    rank of every choice, and tag(*args) with it."""

    def __init__(self, fn, tag=lambda *a: True):
        self.fn, self.tag, self.ranks, self.tags = fn, tag, [], []

    def __call__(self, *a, **k):
        out = self.fn(*a, **k)
        self.ranks.append(int(out[0] if isinstance(out, tuple) else out))
        self.tags.append(bool(self.tag(*a)))
        return out


@functools.lru_cache(maxsize=None)
def _cached_match(sample_plies, rules):
    import fakenet
    import match_model as MM
    from cchess_zero_amd.arena import Openings
    op = Openings(*wide_subset(_STATE["golden"], MATCH_OPENINGS))
    players = [(fakenet.make_forward(m, s), p) for m, s, p in MATCH_PLAYERS]
    spy = _Ranks(MM.choose, lambda visits, ply, sample_plies, seed, game: ply < sample_plies)
    try:
        MM.choose = spy
        want = MM.play_match(players, op, MATCH_PLIES, sample_plies, MATCH_SEED, None, rules)
    finally:
        MM.choose = spy.fn
    return op, want, np.array(spy.ranks), np.array(spy.tags)


def match_reference(rules_golden, sample_plies, rules):
    """match_model.play_match on 10 wide openings, 3 plies per game -> (openings, the model's arrays, the rank of every chosen
    candidate among the candidates of its choice: all root children under "capture", the king-safe ones under "xiangqi"; whether
    that choice was sampled)."""
    reference_roots(rules_golden)
    return _cached_match(sample_plies, rules)


def selfplay_stream(G):
    rng = np.random.default_rng(3)
    return [(rng.gamma(0.3, size=(G, 128)).astype(np.float32), rng.random(G).astype(np.float32)) for _ in range(SP_STEPS)]


@functools.lru_cache(maxsize=None)
def _cached_selfplay():
    import selfplay_model as M
    import selfplay_rules_model as XS
    boards, side, rr = wide_subset(_STATE["golden"], SP_TREES)
    spy = _Ranks(M.choose_ref)
    try:
        M.choose_ref = spy
        want = XS.play_games(net("posabs"), SP_PLAYOUTS, boards, side, rr, selfplay_stream(SP_TREES), max_plies=SP_MAX_PLIES,
                             temperature=1.0, eps=0.25, fold=0)
    finally:
        M.choose_ref = spy.fn
    return (boards, side, rr), want, np.array(spy.ranks)


def selfplay_reference(rules_golden):
    """selfplay_rules_model.play_games at the king-safe level (rules "xiangqi", no repetition rule) on 10 wide roots -> (roots, the
    model's result, the rank of every pick among the king-safe candidates)."""
    reference_roots(rules_golden)
    return _cached_selfplay()
