"""Host model of the evaluation-match kernels of csrc/cz_match.hip (cchess_zero_amd/arena.py).

  uniform        the documented uniform of a sampled ply: splitmix64 of (seed, global game, ply)
  choose         k_match_choose: the first maximum of N (greedy), or softmax(log N) by inverse CDF for the first sample_plies
  adjudicate     k_match_adjudicate's game end: king missing, rr >= 60, ply cap, aborted (no child to play)
  queue          which game a slot starts with, which opening a game plays, who is red
  play_game      one game replayed with one oracle.Search per player and the same follow rule: the mover searches and
                 re-roots on its child, the other player's tree keeps its subtree for the move or starts a fresh root
  device_forward a fakenet forward on device planes (the HIP engines' plain-callable player)
"""
import numpy as np

import fakenet

M64 = (1 << 64) - 1
KING_RED, KING_BLACK = 1, 8
KING, RR60, PLY_CAP, ABORTED = 1, 2, 3, 4


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


def play_game(players, board, side, rr, game, max_plies, sample_plies=0, seed=0, cap=1 << 20):
    """Global game `game` from (board, side, rr): players = [(fwd_a, playouts_a), (fwd_b, playouts_b)] with numpy forwards.
    -> dict(moves, plies, reason, result, a_red)."""
    from oracle import oracle as O
    a_red = game % 2 == 0
    trees = [O.Search(1, cap), O.Search(1, cap)]
    for S in trees:
        S.reset(np.asarray(board, np.uint8)[None], np.array([side], np.uint8), np.array([rr], np.int32))
    moves, ply, side = [], 0, int(side)
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
            mv = int(st["label"][0, choose(st["N"][0, :n], ply, sample_plies, seed, game)])
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
    return dict(moves=moves, plies=ply, reason=reason, result=result, a_red=int(a_red))


def play_match(players, openings, max_plies, sample_plies=0, seed=0, pairs=None):
    """Every game of the given opening pairs (global indices; default all) -> dict of per-game arrays over those games in
    order (2 per pair), moves [n, max_plies] u16 with 0xFFFF past the end."""
    pairs = range(len(openings.boards)) if pairs is None else pairs
    out = dict(result=[], a_red=[], plies=[], reason=[], moves=[])
    for p in pairs:
        for c in (0, 1):
            g = play_game(players, openings.boards[p], int(openings.side[p]), int(openings.rr[p]), 2 * p + c, max_plies,
                          sample_plies, seed)
            row = np.full(max_plies, 0xFFFF, np.uint16)
            row[:len(g["moves"])] = g["moves"]
            for k in ("result", "a_red", "plies", "reason"):
                out[k].append(g[k])
            out["moves"].append(row)
    return dict(result=np.array(out["result"], np.int8), a_red=np.array(out["a_red"], np.uint8), plies=np.array(out["plies"], np.int32),
                reason=np.array(out["reason"], np.uint8), moves=np.array(out["moves"], np.uint16).reshape(-1, max_plies))


def device_forward(mode, salt):
    """fakenet.make_forward(mode, salt) for the HIP engine: device planes [B,9,10,14] f32 -> device (logits, value)."""
    import torch
    f = fakenet.make_forward(mode, salt)

    def forward(planes):
        lg, v = f(planes.float().cpu().numpy())
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    return forward
