"""The model of the perpetual-chase rule (TEST INFRASTRUCTURE), on top of the C oracle's pseudo-legal generator, as
tests/kingsafe_model.py is.  cz_chase.h, cz_threats and cz_repetition_chase are held to this file bit for bit.

threats(board, s): s is the side to move (the possible victim), X = 1 - s the side that just moved.  Square t is threatened
when it holds a piece of s and some pseudo-legal move a -> t of X on this board passes five clauses:
  1  the attacker is a rook, cannon, knight, advisor or bishop (kings and pawns may chase freely);
  2  the victim is not the king and not a pawn on its own side of the river;
  3  the capture is king-safe for X (a pinned piece threatens nothing);
  4  it is no exchange offer: attacker and victim of one kind, and s has the pseudo-legal move t -> a;
  5  the victim is not protected (after a x t, s has a pseudo-legal move onto t — pseudo-legal on purpose: the library's
     definition), unless it is worth more than the attacker (R 3, N = C 2, A = B = P 1).

A chase record of a position is four 64-bit words: the threatened set (bits 0-63, 64-89) and the occupancy of the side to
move in the same layout.  verdict() judges a game history of such records after tests/repetition_model.verdict."""
import numpy as np

import repetition_model as RM
from kingsafe_model import attacked
from oracle import oracle as O

NONE, DRAW, RED_LOSES, BLACK_LOSES = RM.NONE, RM.DRAW, RM.RED_LOSES, RM.BLACK_LOSES
CAUSE_NONE, CAUSE_CHECK, CAUSE_CHASE = 0, 1, 2
K, A, R, B, N, P, C = 1, 2, 3, 4, 5, 6, 7
VALUE = {R: 3, N: 2, C: 2, A: 1, B: 1, P: 1}
MASK64 = (1 << 64) - 1
_SRCDST = None


def _srcdst(labels):
    global _SRCDST
    if _SRCDST is None:
        _SRCDST = O.label_srcdst().astype(np.int64)
    v = _SRCDST[np.asarray(labels, np.int64)]
    return v & 0xFF, v >> 8


def kind(code):
    return (int(code) - 1) % 7 + 1


def threats(board, s, reasons=None):
    """-> the sorted list of threatened squares.  reasons: a dict that counts, per exclusion clause 1 .. 5, the captures it
    took out (a capture is counted at the first clause that excludes it) and under 0 the captures that are threats."""
    board = np.ascontiguousarray(board, np.uint8)
    x = 1 - s
    out = set()
    src, dst = _srcdst(O.legal_moves(board, x))
    back = None

    def count(c):
        if reasons is not None:
            reasons[c] = reasons.get(c, 0) + 1
    for label, a, t in zip(O.legal_moves(board, x), src, dst):
        a, t = int(a), int(t)
        if board[t] == 0:
            continue
        ak, vk = kind(board[a]), kind(board[t])
        if ak in (K, P):
            count(1); continue
        if vk == K or (vk == P and (t // 9 <= 4 if s == 0 else t // 9 >= 5)):
            count(2); continue
        after = O.apply_move(board, int(label))[0]
        if attacked(after, x):
            count(3); continue
        if ak == vk:
            if back is None:
                bs, bd = _srcdst(O.legal_moves(board, s))
                back = set(zip(bs.tolist(), bd.tolist()))
            if (t, a) in back:
                count(4); continue
        _, pd = _srcdst(O.legal_moves(after, s))
        if (pd == t).any() and VALUE[vk] <= VALUE[ak]:
            count(5); continue
        count(0)
        out.add(t)
    return sorted(out)


def bits(squares):
    v = 0
    for q in squares:
        v |= 1 << int(q)
    return v


def record(board, s):
    """-> the chase record of a position: [threat lo, threat hi, own lo, own hi] as Python ints"""
    board = np.asarray(board)
    t = bits(threats(board, s))
    own = bits(np.nonzero((board >= 8) if s else ((board >= 1) & (board <= 7)))[0])
    return [t & MASK64, t >> 64, own & MASK64, own >> 64]


def records(boards, side):
    """-> [n, 4] uint64"""
    return np.array([record(b, int(s)) for b, s in zip(boards, side)], np.uint64).reshape(-1, 4)


def chases(recs, reached):
    """recs[i]: the record of position i; reached: the positions after one side's moves, in game order -> that side chases
    perpetually: one and the same piece is threatened in every one of them."""
    if len(reached) == 0:
        return False
    T = lambda i: int(recs[i][0]) | (int(recs[i][1]) << 64)
    own = lambda i: int(recs[i][2]) | (int(recs[i][3]) << 64)
    c = T(reached[0])
    for prev, i in zip(reached, reached[1:]):
        frm, to = own(prev) & ~own(i), own(i) & ~own(prev)
        if bin(frm).count("1") == 1 and bin(to).count("1") == 1:     # the victim side moved one piece and nothing was taken
            if c & frm:
                c = (c & ~frm) | to
        else:
            c = 0
        c &= T(i)
    return c != 0


def verdict(keys, in_check, recs, side_now, window=None, fold=3):
    """keys / in_check / recs: positions 0 .. n, the last one current, side_now to move in it -> (code, first, cause)"""
    code, j = RM.verdict(keys, in_check, side_now, window, fold)
    if code == NONE:
        return NONE, -1, CAUSE_NONE
    if code != DRAW:
        return code, j, CAUSE_CHECK
    n = len(keys) - 1
    side = lambda i: (side_now ^ (n - i)) & 1
    cycle = range(j + 1, n + 1)
    if any(len([i for i in cycle if side(i) == 1 - x]) > 0 and all(bool(in_check[i]) for i in cycle if side(i) == 1 - x) for x in (0, 1)):
        return DRAW, j, CAUSE_NONE                                     # both sides checked perpetually
    chase = [chases(recs, [i for i in cycle if side(i) == 1 - x]) for x in (0, 1)]
    if chase[0] == chase[1]:
        return DRAW, j, CAUSE_NONE
    return (RED_LOSES if chase[0] else BLACK_LOSES), j, CAUSE_CHASE


def mirror(board):
    """The same position with the colours swapped: ranks reversed, red <-> black"""
    b = np.asarray(board, np.uint8).reshape(10, 9)[::-1].reshape(-1).copy()
    red, black = (b >= 1) & (b <= 7), b >= 8
    b[red] += 7
    b[black] -= 7
    return b


def mirror_sq(q):
    return 9 * (9 - q // 9) + q % 9


_CACHE = {}


def reference(name, boards_side):
    """The model's records of a named corpus, computed once per process and shared by the tests that need them (read-only):
    boards_side() -> (boards, side) is called on the first request -> (boards, side, records [n, 4] uint64)"""
    if name not in _CACHE:
        boards, side = boards_side()
        recs = records(boards, side)
        for a in (boards, side, recs):
            a.setflags(write=False)
        _CACHE[name] = (boards, side, recs)
    return _CACHE[name]


def corpus_reference():
    from kingsafe_model import playout_corpus
    return reference("corpus", lambda: tuple(np.ascontiguousarray(a) for a in playout_corpus()))


def table_reference():
    import chase_cases as CC
    return reference("table", lambda: (np.stack([c[1] for c in CC.TABLE]), np.array([c[2] for c in CC.TABLE], np.uint8)))


def golden_reference(rules_golden):
    return reference("golden", lambda: (np.ascontiguousarray(rules_golden["boards"]), np.ascontiguousarray(rules_golden["side"], np.uint8)))
