"""The model of king-safe move generation (TEST INFRASTRUCTURE), on top of the C oracle's pseudo-legal generator.

attacked(board, s): side s has a king and the other side has a pseudo-legal move (oracle.legal_moves: the reference's
get_legal_moves, flying general included) onto its square.  A pseudo-legal move is king-safe iff the mover's king is not
attacked after it — one uniform rule.  cz_kingsafe.h and cz_movegen_kingsafe are held to this file bit for bit."""
import numpy as np

from oracle import oracle as O

IN_CHECK, CAN_TAKE_KING, NO_SAFE_MOVE = 1, 2, 4
_DST = None


def _dst(label):
    global _DST
    if _DST is None:
        _DST = (O.label_srcdst() >> 8).astype(np.int64)
    return _DST[label]


def attacked(board, s):
    king = np.nonzero(np.asarray(board) == (8 if s else 1))[0]
    if len(king) == 0:
        return False
    return bool((_dst(O.legal_moves(board, 1 - s)) == king[0]).any())


def kingsafe(board, side):
    """-> (the king-safe labels in the reference's order, np.uint16; the position flags)"""
    pseudo = O.legal_moves(board, side)
    safe = np.array([m for m in pseudo if not attacked(O.apply_move(board, int(m))[0], side)], np.uint16)
    flags = (IN_CHECK if attacked(board, side) else 0) | (CAN_TAKE_KING if attacked(board, 1 - side) else 0) | (0 if len(safe) else NO_SAFE_MOVE)
    return safe, flags


def mask_of(moves):
    m = np.zeros(66, np.uint32)
    for l in moves:
        m[int(l) >> 5] |= np.uint32(1) << np.uint32(int(l) & 31)
    return m


def model_batch(boards, side):
    """-> (lists, counts int32, masks [n, 66], flags uint8, pseudo counts) of the model for every position"""
    lists, flags, pseudo = [], [], []
    for b, s in zip(boards, side):
        mv, f = kingsafe(b, int(s))
        lists.append(mv); flags.append(f); pseudo.append(len(O.legal_moves(b, int(s))))
    masks = np.stack([mask_of(l) for l in lists])
    return lists, np.array([len(l) for l in lists], np.int32), masks, np.array(flags, np.uint8), np.array(pseudo, np.int32)


def shares(counts, flags, pseudo):
    """(in check, king-safe != pseudo-legal, no king-safe move, mover can take the king) as position counts"""
    return (int((flags & IN_CHECK != 0).sum()), int((counts != pseudo).sum()), int((flags & NO_SAFE_MOVE != 0).sum()), int((flags & CAN_TAKE_KING != 0).sum()))


def playout_corpus(games=60, max_ply=120, seed=2024):
    """Seeded uniform random playouts from the start position under the reference's rules, each continued until a king falls
    (or max_ply): every position on the way, the one without a king included."""
    rng = np.random.default_rng(seed)
    boards, sides = [], []
    for _ in range(games):
        b, s = O.fen_to_board(O.START_FEN), 0
        for _ply in range(max_ply):
            boards.append(b.copy()); sides.append(s)
            mv = O.legal_moves(b, s)
            if len(mv) == 0 or not (b == 1).any() or not (b == 8).any():
                break
            b = O.apply_move(b, int(mv[rng.integers(len(mv))]))[0]
            s ^= 1
    return np.stack(boards), np.array(sides, np.uint8)
