"""Host model of the evaluation-match kernels of csrc/cz_match.hip (cchess_zero_amd/arena.py).

  uniform        the documented uniform of a sampled ply: splitmix64 of (seed, global game, ply)
  choose         k_match_choose: the first maximum of N (greedy), or softmax(log N) by inverse CDF for the first sample_plies
  choose_safe    choose over the king-safe root children (rules="xiangqi")
  ending         a verdict of the repetition or chase rule as (reason, result for A)
  adjudicate     k_match_adjudicate's game end (wave_game_end, csrc/cz_internal.h): aborted (no child to play), king missing,
                 rr >= 60, ply cap
  queue          which game a slot starts with, which opening a game plays, who is red
  play_game      one game replayed with one oracle.Search per player and the same follow rule: the mover searches and
                 re-roots on its child, the other player's tree keeps its subtree for the move or starts a fresh root; at
                 every rule level of tests/rootrules_model.py, whose steps stand in front of the choice
  fakenet_match  the 16-game fixture match of the rules tests, replayed once per process and level
  device_forward a fakenet forward on device planes (the HIP engines' plain-callable player)
"""
import functools

import numpy as np

import chase_model as CM
import fakenet
import repetition_cases as RC
import repetition_model as RM
import rootrules_model as RR

M64 = (1 << 64) - 1
KING_RED, KING_BLACK = 1, 8
KING, RR60, PLY_CAP, ABORTED, MATE, REPETITION, PERPETUAL, CHASE = 1, 2, 3, 4, 5, 6, 7, 9


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniform(seed, game, ply):
    """u in [0, 1) of ply `ply` of global game `game` (include/cchess_hip.h cz_match_choose)."""
    h = splitmix64((int(seed) & M64) ^ splitmix64(((int(game) << 16) | int(ply)) & M64))
    return (h >> 11) * 2.0 ** -53


def visit_pi(visits):
    """softmax(log N) (temperature 1, main.py:1341) with the kernel's uniform fallback when nothing was visited."""
    v = np.asarray(visits, np.int64)
    if not v.any():
        return np.full(len(v), 1.0 / len(v))
    with np.errstate(divide="ignore"):
        x = np.log(v.astype(np.float64))
    e = np.exp(x - x.max())
    return e / e.sum()


def choose(visits, ply, sample_plies, seed, game):
    """-> child index: greedy (first maximum of N in generation order) or, for ply < sample_plies, the inverse CDF of
    softmax(log N) at the game's uniform."""
    visits = np.asarray(visits, np.int64)
    if ply >= sample_plies:
        return int(np.argmax(visits))          # np.argmax: the first maximum
    p = visit_pi(visits)
    c = np.cumsum(p)
    target = uniform(seed, game, ply) * c[-1]
    hit = np.nonzero((p > 0) & (c > target))[0]
    return int(hit[0]) if len(hit) else int(np.nonzero(p > 0)[0][-1])


def choose_safe(board, side, labels, visits, ply, sample_plies, seed, game):
    """-> child index among all children (choose over the king-safe ones), or None: no king-safe child."""
    idx = RR.safe_children(board, side, labels)
    if not idx:
        return None
    return idx[choose(np.asarray(visits)[idx], ply, sample_plies, seed, game)]


def ending(code, cause, a_red):
    """A verdict of the rule -> (reason, result for A): a chase is scored like a perpetual check, with its own reason."""
    if code == RM.DRAW:
        return REPETITION, 0
    return (CHASE if cause == CM.CAUSE_CHASE else PERPETUAL), (-1 if (code == RM.RED_LOSES) == bool(a_red) else 1)


def adjudicate(board, rr, ply, max_plies, aborted, a_red):
    """-> (reason, result for A) after a move, or (0, 0) while the game goes on."""
    if aborted:
        return ABORTED, 0
    board = np.asarray(board)
    K, k = (board == KING_RED).any(), (board == KING_BLACK).any()
    if not K or not k:
        red_wins = not k                       # 'k' missing: red ("w") wins, main.py:1384-1389
        return KING, (1 if red_wins == bool(a_red) else -1)
    if rr >= 60:
        return RR60, 0
    if ply >= max_plies:
        return PLY_CAP, 0
    return 0, 0


def queue(n_openings, G):
    """Game i plays opening i // 2 with A red when i is even; slot g starts game g (g < games), the rest of the queue is
    handed out in order as games end.  -> (opening [games], a_red [games], first game of each slot [G], -1 = parked)."""
    n = 2 * n_openings
    games = np.arange(n)
    return games // 2, (games % 2 == 0).astype(np.uint8), np.where(np.arange(G) < n, np.arange(G), -1)


def _search(S, fwd, playouts):
    """SearchEngine.search on one oracle tree: the root step, then `playouts` simulations."""
    for step in range(playouts + 1):
        planes, need = S.select(0 if step == 0 else 1)
        logits = np.zeros((1, 2086), np.float32)
        value = np.zeros((1, 1), np.float32)
        if need[0]:
            logits, value = fwd(planes)
        S.expand_backup(logits, value)


def play_game(players, board, side, rr, game, max_plies, sample_plies=0, seed=0, rules="capture", fold=0, chase=False, cap=1 << 20, trace=None,
              preset=None):
    """Global game `game` from (board, side, rr): players = [(fwd_a, playouts_a), (fwd_b, playouts_b)] with numpy forwards, at
    the rule level of (rules, fold, chase).  -> dict(moves, plies, reason, result, a_red), and records (the chase records of the
    roots) at the chase level.  trace (a list): receives (ply, first) of the game's verdict, (ply, first, cause) at the chase level.
    preset: hand-set ring keys (rootrules_model.History)."""
    from oracle import oracle as O
    level = RR.level(rules, fold, chase)
    a_red = game % 2 == 0
    trees = [O.Search(1, cap), O.Search(1, cap)]
    for S in trees:
        S.reset(np.asarray(board, np.uint8)[None], np.array([side], np.uint8), np.array([rr], np.int32))
    moves, ply, side = [], 0, int(side)
    history = RR.History(level, fold, preset=preset)
    try:
        while True:
            mover = 0 if (side == 0) == a_red else 1
            S = trees[mover]
            _search(S, *players[mover])
            st = S.root_stats()
            n = int(st["count"][0])
            status = int(S.status()[0][0])
            if n == 0 or status & (2 | 4):
                reason, result = adjudicate(None, 0, ply, max_plies, True, a_red)
                break
            b, s, r = S.root_state()
            if level >= RR.REPETITION:
                code, first, cause = history.root(b[0], side, r[0], ply)
                if code != RM.NONE:
                    if trace is not None:
                        trace.append((ply, first, cause) if level >= RR.CHASE else (ply, first))
                    reason, result = ending(code, cause, a_red)
                    break
            if level >= RR.KINGSAFE:
                pick = choose_safe(b[0], side, st["label"][0, :n], st["N"][0, :n], ply, sample_plies, seed, game)
                if pick is None:                    # the mover has children, none king-safe: it loses
                    reason, result = MATE, (-1 if mover == 0 else 1)
                    break
            else:
                pick = choose(st["N"][0, :n], ply, sample_plies, seed, game)
            mv = int(st["label"][0, pick])
            moves.append(mv)
            ply += 1
            for T in trees:            # the mover re-roots on its child, the other keeps its subtree or starts afresh
                T.advance(np.array([mv], np.uint16))
            b, s, r = S.root_state()
            side = int(s[0])
            reason, result = adjudicate(b[0], int(r[0]), ply, max_plies, False, a_red)
            if reason:
                break
    finally:
        for T in trees:
            T.close()
    g = dict(moves=moves, plies=ply, reason=reason, result=result, a_red=int(a_red))
    return dict(g, records=history.records) if level >= RR.CHASE else g


def play_match(players, openings, max_plies, sample_plies=0, seed=0, pairs=None, rules="capture", fold=0, chase=False):
    """Every game of the given opening pairs (global indices; default all) of openings (.boards / .side / .rr) -> dict of per-game
    arrays over those games in order (2 per pair), moves [n, max_plies] u16 with 0xFFFF past the end."""
    pairs = range(len(openings.boards)) if pairs is None else pairs
    games = [play_game(players, openings.boards[p], int(openings.side[p]), int(openings.rr[p]), 2 * p + c, max_plies, sample_plies, seed,
                       rules, fold, chase) for p in pairs for c in (0, 1)]
    moves = np.full((len(games), max_plies), 0xFFFF, np.uint16)
    for row, g in zip(moves, games):
        row[:len(g["moves"])] = g["moves"]
    col = lambda k, dtype: np.array([g[k] for g in games], dtype)
    return dict(result=col("result", np.int8), a_red=col("a_red", np.uint8), plies=col("plies", np.int32), reason=col("reason", np.uint8),
                moves=moves)


@functools.lru_cache(maxsize=None)
def fakenet_openings():
    """The 8 openings of the 16-game fixture match, made on the CPU (repetition_cases.cpu_openings(8, 4, 11)); read-only."""
    from cchess_zero_amd.arena import Openings
    return Openings(*RC.cpu_openings(8, 4, 11))


@functools.lru_cache(maxsize=None)
def _fakenet_match(sample_plies, rules, fold, chase):
    players = [(fakenet.make_forward("pos", 11), 24), (fakenet.make_forward("signed", 12), 16)]
    out = play_match(players, fakenet_openings(), 160, sample_plies, 5, None, rules, fold, chase)
    for a in out.values():
        a.setflags(write=False)
    return out


def fakenet_match(sample_plies, rules="xiangqi", fold=3, chase=True):
    """The 16-game fixture match (fakenet_openings(), pos/11 at 24 playouts against signed/12 at 16, max_plies 160, seed 5) at
    the rule level of (rules, fold, chase), replayed on the CPU once per process and level; read-only."""
    return _fakenet_match(sample_plies, rules, fold, chase)


def assert_equals_model(res, want, tag=None):
    """A finished arena.MatchResult against play_match's arrays: every per-game array and every game's moves."""
    from cchess_zero_amd._lib import tables
    lab = tables()["labels"]
    for k in ("a_red", "plies", "reason", "result"):
        assert np.array_equal(getattr(res, k), want[k]), (tag, k, getattr(res, k), want[k])
    assert len(res.moves) == len(want["moves"])
    for g, row in enumerate(want["moves"]):
        assert res.moves[g] == [lab[int(x)] for x in row if x != 0xFFFF], (tag, g)
    assert res.unfinished == 0


def device_forward(mode, salt):
    """fakenet.make_forward(mode, salt) for the HIP engine: device planes [B,9,10,14] f32 -> device (logits, value)."""
    import torch
    f = fakenet.make_forward(mode, salt)

    def forward(planes):
        lg, v = f(planes.float().cpu().numpy())
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    return forward
