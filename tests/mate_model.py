"""The model of the forced-mate search (TEST INFRASTRUCTURE), in Python and numpy alone, on kingsafe_model (the C oracle's
pseudo-legal generator filtered by the model's attack rule) and perft_model.make_move.  Nothing here touches cz_kingsafe.h or
any kernel: cz_movegen_checks, cz_mate_backup and Rules.mate are held to this file bit for bit.

    checks(board, side)   the king-safe moves after which the other side is attacked, in list order
    backup(...)           cz_mate_backup's contract in numpy
    solve(...)            the recursive AND/OR search: the side to move attacks, `plies` odd; dist = plies until the defender
                          is mated; an attacker takes the FIRST child with the smallest distance, a defender the FIRST with the
                          largest; a defender without a king-safe move is mated (dist 0), one at the horizon is not proven.

`PYTHONPATH=. python tests/mate_model.py` rewrites tests/golden/mate_playouts.npz: the model's answers on the playout corpus
and on the open-board subset, which the GPU tests read instead of running the model for a minute and a half
(tests/test_mate_model_cpu.py holds the file to a fresh run of the model)."""
import os

import numpy as np

import kingsafe_model as M
from perft_model import leaf_flags, make_move

NONE = 0x7FFF
NO_MATE, MATE, BAD_ROOT, LIMIT = 0, 1, 2, 3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mate_playouts.npz")
GOLDEN_PLIES = (1, 3, 5)


def checks(board, side):
    """-> (the king-safe labels that give check, in the king-safe list's order, np.uint16; the position's own flags)"""
    safe, flags = M.kingsafe(board, side)
    return np.array([m for m in safe if M.attacked(make_move(board, m)[0], 1 - side)], np.uint16), flags


def backup(offsets, total, child_dist, child_label, child_pv, W, mode):
    """-> (out_dist int16 [G], out_pv uint16 [G, W + 1]); offsets clamped into [0, total] as cz_successors clamps them"""
    G = len(offsets) - 1
    out_dist, out_pv = np.full(G, NONE, np.int16), np.full((G, W + 1), 0xFFFF, np.uint16)
    for g in range(G):
        c0 = min(max(int(offsets[g]), 0), total)
        c1 = min(max(int(offsets[g + 1]), c0), total)
        d = np.asarray(child_dist[c0:c1]).astype(np.int64)
        proven = (d >= 0) & (d < NONE)
        best, dist = None, NONE
        if mode == 0:
            if proven.any():
                best = int(np.argmin(np.where(proven, d, NONE)))          # argmin / argmax: the first occurrence
                dist = int(d[best]) + 1
        elif len(d) == 0:
            dist = 0
        elif proven.all():
            best = int(np.argmax(d))
            dist = int(d[best]) + 1
        out_dist[g] = dist
        if best is not None and dist != NONE:
            out_pv[g, 0] = child_label[c0 + best]
            if W:
                out_pv[g, 1:] = child_pv[c0 + best]
    return out_dist, out_pv


def bad_root(board, side):
    """A king is missing, or the mover can already take the king"""
    board = np.asarray(board)
    return not (board == 1).any() or not (board == 8).any() or M.attacked(board, 1 - side)


def solve(board, side, plies, mode="checks"):
    """-> (status, dist, pv): status NO_MATE / MATE / BAD_ROOT, dist the plies to the mate (NONE without one), pv uint16
    [plies], 0xFFFF behind the line.  mode "checks": the attacker plays checking moves only; "all": every king-safe move."""
    assert plies % 2 == 1 and mode in ("checks", "all")
    board, side = np.asarray(board, np.uint8), int(side)
    pv = np.full(plies, 0xFFFF, np.uint16)
    if bad_root(board, side):
        return BAD_ROOT, NONE, pv

    def attack(b, s, p):
        moves = checks(b, s)[0] if mode == "checks" else M.kingsafe(b, s)[0]
        best, line = NONE, []
        for m in moves:
            d, l = defend(make_move(b, m)[0], 1 - s, p - 1)
            if d != NONE and d + 1 < best:
                best, line = d + 1, [int(m)] + l
        return best, line

    def defend(b, s, p):
        if p == 0:
            return (0 if leaf_flags(b, s) & M.NO_SAFE_MOVE else NONE), []
        worst, line = -1, []
        for m in M.kingsafe(b, s)[0]:
            d, l = attack(make_move(b, m)[0], 1 - s, p - 1)
            if d == NONE:
                return NONE, []
            if d > worst:
                worst, line = d, [int(m)] + l
        return worst + 1, line

    dist, line = attack(board, side, plies)
    pv[:len(line)] = line
    return (MATE if dist != NONE else NO_MATE), dist, pv


def solve_batch(boards, side, plies, mode="checks"):
    """-> (status uint8 [n], dist int16 [n], pv uint16 [n, plies])"""
    out = [solve(b, s, plies, mode) for b, s in zip(boards, side)]
    return (np.array([o[0] for o in out], np.uint8), np.array([o[1] for o in out], np.int16),
            np.stack([o[2] for o in out]) if out else np.zeros((0, plies), np.uint16))


def legal_roots(boards, side):
    """The indices of the positions that are no bad root"""
    return np.array([i for i in range(len(boards)) if not bad_root(boards[i], int(side[i]))], np.int64)


def open_subset():
    """The roots the "all" mode is held to: conftest.open_boards(900, 12)'s legal roots with at most 60 king-safe moves and at most
    three pieces of the other side (71 positions; the model solves them at 3 plies in ~25 s, where 567 full boards took 12
    minutes) -> (boards, side)"""
    from conftest import open_boards
    boards, side = open_boards(900, 12)
    keep = []
    for i in legal_roots(boards, side):
        b, s = boards[i], int(side[i])
        other = (b > 0) & ((b > 7) == (s == 0))
        if len(M.kingsafe(b, s)[0]) <= 60 and int(other.sum()) <= 3:
            keep.append(i)
    return boards[keep], side[keep]


def open_solutions():
    """The recorded answers of solve() at 3 plies on open_subset() -> {"all": (status, dist, pv), "checks": ...}"""
    z = np.load(GOLDEN)
    return {m: (z["open_%s_status" % m], z["open_%s_dist" % m], z["open_%s_pv" % m]) for m in ("all", "checks")}


def playout_solutions():
    """The recorded answers of solve() in "checks" mode on M.playout_corpus() (every position, bad roots included) ->
    {plies: (status, dist, pv)}"""
    z = np.load(GOLDEN)
    return {p: (z["status%d" % p], z["dist%d" % p], z["pv%d" % p]) for p in GOLDEN_PLIES}


if __name__ == "__main__":
    boards, side = M.playout_corpus()
    out = {}
    for p in GOLDEN_PLIES:
        out["status%d" % p], out["dist%d" % p], out["pv%d" % p] = solve_batch(boards, side, p)
        print("plies %d: %d mates" % (p, int((out["status%d" % p] == MATE).sum())))
    boards, side = open_subset()
    for m in ("all", "checks"):
        out["open_%s_status" % m], out["open_%s_dist" % m], out["open_%s_pv" % m] = solve_batch(boards, side, 3, m)
        print("open subset, %s: %d roots, %d mates in 1 ply, %d in 3" % (m, len(boards), int((out["open_%s_dist" % m] == 1).sum()), int((out["open_%s_dist" % m] == 3).sum())))
    np.savez_compressed(GOLDEN, **out)
