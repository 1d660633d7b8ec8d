"""Host model (float64) of the self-play bookkeeping kernels of csrc/cz_selfplay.hip.

  choose_ref      k_sp_choose's pick: cchess_main.get_action (main.py:1339-1348) with np.random.choice's inverse CDF driven
                  by an explicit uniform, plus the kernel's two documented departures (all-zero visits, gamma summing to 0)
  adjudicate_ref  k_sp_adjudicate's game-end test (wave_game_end, csrc/cz_internal.h): cchess_main.selfplay
                  (main.py:1525-1545) plus the documented extensions of include/cchess_hip.h (max_plies draw, stalled games)
  stats_ref       the cz_selfplay_stats counters of a list of finished games
  flush_ref       k_sp_flush: finished games' records into the ring, modulo ring_records, dropped whole past read_cursor
  golden_stream   a golden game's own numpy stream: per ply the Dirichlet vector and the uniform np.random.choice draws
"""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RED, BLACK = 0, 1          # side codes: "w" moves first, "b" second
KING_RED, KING_BLACK = 1, 8  # piece codes of 'K' and 'k'


def visit_probs(visits, temperature):
    """softmax(1.0 / temperature * np.log(visits)) with the reference's softmax (main.py:1111-1116, :1341)."""
    with np.errstate(divide="ignore"):
        x = 1.0 / temperature * np.log(np.asarray(visits, np.int64))
    probs = np.exp(x - np.max(x))
    probs /= np.sum(probs)
    return probs


def choice_probs(visits, temperature, gamma, eps):
    """-> p [k] float64: what k_sp_choose samples from."""
    visits = np.asarray(visits, np.int64)
    k = len(visits)
    if not visits.any():
        # departure 1: with no visit at all the reference's softmax is NaN (np.random.choice raises); the kernel plays uniformly
        pi = np.full(k, 1.0 / k)
    else:
        pi = visit_probs(visits, temperature)
    g = None if gamma is None else np.asarray(gamma, np.float64)[:k]
    if eps == 0 or g is None or g.sum() == 0.0:
        # departure 2: no noise when it is off or when gamma sums to 0 over the children (nothing to normalise)
        return pi
    # 0.75 * probs + 0.25 * np.random.dirichlet(0.3 * np.ones(len(probs))), main.py:1346 (eps = 0.25)
    return (1.0 - eps) * pi + eps * (g / g.sum())


def choose_ref(visits, temperature, gamma, eps, u):
    """-> (child index, margin): np.random.choice(k, p=p) given the uniform `u` it would draw (numpy's own inverse CDF:
    cdf = p.cumsum(); cdf /= cdf[-1]; searchsorted(cdf, u, 'right')).  margin = distance from u to the nearest CDF boundary
    strictly inside (0, 1); inf for the exact cases (u = 0: the first positive child; u >= 1: the fallback below).
    An array of uniforms gives arrays (one tree, many draws)."""
    p = choice_probs(visits, temperature, gamma, eps)
    cdf = p.cumsum()
    cdf /= cdf[-1]
    uu = np.atleast_1d(np.asarray(u, np.float64))
    i = np.searchsorted(cdf, uu, side="right")
    over = i >= len(p)
    # the kernel's rounding fallback at the top of the CDF: the last child with a positive probability
    i = np.where(over, np.nonzero(p > 0)[0][-1], i)
    inner = cdf[:-1][(cdf[:-1] > 0) & (cdf[:-1] < 1)]
    margin = np.abs(inner[None, :] - uu[:, None]).min(axis=1) if len(inner) else np.full(len(uu), np.inf)
    margin[over | (uu == 0)] = np.inf
    if np.ndim(u) == 0:
        return int(i[0]), float(margin[0])
    return i, margin


def intervals(visits, temperature, gamma, eps):
    """-> (p, lo, hi): child i is picked for lo[i] <= u < hi[i] (normalised CDF, float64)."""
    p = choice_probs(visits, temperature, gamma, eps)
    hi = p.cumsum()
    hi /= hi[-1]
    lo = np.concatenate([[0.0], hi[:-1]])
    return p, lo, hi


class Outcome:
    """A finished game as k_sp_adjudicate ends it: result in {"red", "black", "draw", "stalled"}, fin_n records, their z."""

    def __init__(self, result, fin_n, z):
        self.result, self.fin_n, self.z = result, int(fin_n), np.asarray(z, np.int8)

    def __repr__(self):
        return "Outcome(%s, %d)" % (self.result, self.fin_n)


def adjudicate_ref(board, rr, ply, movers, max_plies, stalled=False):
    """The game-end tests after a move.  board / rr: the position after it; ply: plies played so far; movers: the side of
    every recorded ply.  -> Outcome, or None while the game goes on."""
    if stalled:
        # no child to play, or a move that is not a root child (BAD_ADVANCE): dropped with no record
        return Outcome("stalled", 0, [])
    n = min(int(ply), int(max_plies))      # records kept: the history holds max_plies of them
    movers = np.asarray(movers, np.int64)[:n]
    board = np.asarray(board)
    K, k = (board == KING_RED).any(), (board == KING_BLACK).any()
    if not K or not k:                      # main.py:1532-1541
        if not K:
            winner = BLACK                  # 'K' missing: "b" wins
        if not k:
            winner = RED                    # 'k' missing: "w" wins
        return Outcome("red" if winner == RED else "black", n, np.where(movers == winner, 1, -1))
    if rr >= 60:                            # main.py:1542-1545: a tie, z = 0
        return Outcome("draw", n, np.zeros(n))
    if ply >= max_plies:                    # the history is full: a draw (the reference has no such limit)
        return Outcome("draw", n, np.zeros(n))
    return None


def stats_ref(outcomes):
    """cz_selfplay_stats slots games .. stalled of the finished games (include/cchess_hip.h CZ_SP_*)."""
    res = [o.result for o in outcomes]
    return dict(games=len(res), red_wins=res.count("red"), black_wins=res.count("black"), draws=res.count("draw"),
                plies=sum(o.fin_n for o in outcomes), stalled=res.count("stalled"))


def flush_ref(ring, hist, fin_n, offset, read_cursor=None):
    """k_sp_flush: game g's records hist[g][:fin_n[g]] go to ring rows (offset[g] + j) % len(ring); a game whose last record
    would pass read_cursor + len(ring) (overwrite rows nobody has drained) is dropped whole.  -> (new ring, dropped)."""
    out = np.array(ring, copy=True)
    R = out.shape[0]
    dropped = 0
    for g, n in enumerate(fin_n):
        n, off = int(n), int(offset[g])
        if n <= 0:
            continue
        if read_cursor is not None and off + n - int(read_cursor) > R:
            dropped += n
            continue
        for j in range(n):
            out[(off + j) % R] = hist[g][j]
    return out, dropped


def golden_games():
    """tests/golden/selfplay.npz as one dict per game (meta, state, side, played, count, labels, visits, z)."""
    g = np.load(os.path.join(GOLDEN, "selfplay.npz"))
    meta = json.loads(str(g["meta"]))
    out = []
    for ci, m in enumerate(meta):
        rows = np.nonzero(g["case"] == ci)[0]
        out.append(dict(meta=m, state=g["state"][rows], side=g["side"][rows], played=g["played"][rows], count=g["count"][rows],
                        labels=g["labels"][rows], visits=g["visits"][rows], z=g["z"][rows]))
    return out


def replay_golden(c, max_plies=512):
    """A golden game on the oracle's boards (states un-flipped, the played labels applied, restrict_round counted from
    meta.rr0): -> (boards before every ply [n, 90], adjudicate_ref after every ply)."""
    from oracle import oracle as O
    from cchess_zero_amd.selfplay import canonical_boards
    board = canonical_boards(c["state"], c["side"])       # canonical states: black's are flipped (an involution)
    rr = c["meta"].get("rr0", 0)
    out = []
    for ply in range(len(board)):
        nb, cap, _ = O.apply_move(board[ply], int(c["played"][ply]))
        rr = 0 if cap else rr + 1
        out.append(adjudicate_ref(nb, rr, ply + 1, c["side"][:ply + 1], max_plies))
        if ply + 1 < len(board):
            assert np.array_equal(nb, board[ply + 1]), (c["meta"]["name"], ply)
    return board, out


def golden_stream(seed, counts):
    """The random numbers a golden game consumed: np.random.seed(seed), then per ply np.random.dirichlet(0.3 * ones(k))
    (main.py:1346) and the one random_sample() inside np.random.choice.  -> list of (dirichlet [k] float64, u float64)."""
    rs = np.random.RandomState(seed)
    out = []
    for k in counts:
        d = rs.dirichlet(0.3 * np.ones(int(k)))
        out.append((d, rs.random_sample()))
    return out
