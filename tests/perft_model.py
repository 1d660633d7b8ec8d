"""The model of cz_successors and of perft under Xiangqi rules (TEST INFRASTRUCTURE), in Python and numpy alone: the moves
are kingsafe_model.kingsafe's (the C oracle's pseudo-legal generator filtered by the model's attack rule), a move is made
by three lines of numpy.  Nothing here touches cz_kingsafe.h or any kernel, so an agreement with the host perft, with the
fixture's published numbers and with Rules.perft is an agreement between independent implementations."""
import numpy as np

import kingsafe_model as M
from oracle import oracle as O

_SRCDST = None


def make_move(board, label):
    """-> (the board after the move, the piece code it took or 0); a label >= 2086 leaves the board"""
    global _SRCDST
    if _SRCDST is None:
        _SRCDST = O.label_srcdst().astype(np.int64)
    child = np.array(board, np.uint8)
    if int(label) >= len(_SRCDST):
        return child, 0
    src, dst = int(_SRCDST[int(label)]) & 0xFF, int(_SRCDST[int(label)]) >> 8
    cap = int(child[dst])
    child[dst], child[src] = child[src], 0
    return child, cap


def successors(boards, side, moves, count):
    """cz_successors' contract in numpy: moves [G, 128] uint16 and count [G] (0xFFFF / -1: no children) -> (boards [T, 90] u8,
    side [T] u8, captured [T] u8, parent [T] i32, label [T] u16, offsets [G + 1] i32): child offsets[g] + j is parent g after
    moves[g][j], in list order, its side 1 - the parent's."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 90)
    cnt = np.asarray(count).astype(np.int64) & 0xFFFF
    cnt[cnt == 0xFFFF] = 0
    offsets = np.zeros(len(boards) + 1, np.int64)
    np.cumsum(cnt, out=offsets[1:])
    T = int(offsets[-1])
    out = (np.zeros((T, 90), np.uint8), np.zeros(T, np.uint8), np.zeros(T, np.uint8), np.zeros(T, np.int32), np.zeros(T, np.uint16))
    for g in range(len(boards)):
        for j in range(int(cnt[g])):
            c = int(offsets[g]) + j
            out[0][c], out[2][c] = make_move(boards[g], moves[g][j])
            out[1][c], out[3][c], out[4][c] = 0 if side[g] else 1, g, moves[g][j]
    return out + (offsets.astype(np.int32),)


def leaf_flags(board, side):
    """kingsafe_model's IN_CHECK and NO_SAFE_MOVE of a position whose moves nobody asks for: the same two definitions, the
    search for a king-safe move stopped at the first one"""
    safe = any(not M.attacked(make_move(board, m)[0], side) for m in O.legal_moves(board, side))
    return (M.IN_CHECK if M.attacked(board, side) else 0) | (0 if safe else M.NO_SAFE_MOVE)


def perft(board, side, depth):
    """-> dict of int64 arrays [depth + 1]: nodes, captures, checks, mates (column 0 the root), every ply made"""
    t = {k: np.zeros(depth + 1, np.int64) for k in ("nodes", "captures", "checks", "mates")}

    def walk(b, s, d, cap):
        moves, flags = M.kingsafe(b, s) if d < depth else (None, leaf_flags(b, s))
        t["nodes"][d] += 1
        t["captures"][d] += 1 if cap else 0
        t["checks"][d] += 1 if flags & M.IN_CHECK else 0
        t["mates"][d] += 1 if flags & M.NO_SAFE_MOVE else 0
        if d < depth:
            for m in moves:
                child, taken = make_move(b, m)
                walk(child, 1 - s, d + 1, taken)
    walk(np.asarray(board, np.uint8), int(side), 0, 0)
    return t
