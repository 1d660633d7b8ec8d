"""tests/kingsafe_model.py (what "in check", "king-safe move" and "no safe move" mean for this library) on positions written by
hand.  Board convention: rank 0, the first row of the state string, is red's home (upper case); square = 9 y + x."""
import numpy as np

import kingsafe_model as M
from oracle import oracle as O


def _pos(rows):
    assert len(rows) == 10
    return O.fen_to_board("/".join(rows))


def _label(src, dst):
    """(y, x) -> (y, x) as a label"""
    l = int(O.lut()[src[0] * 9 + src[1], dst[0] * 9 + dst[1]])
    assert l >= 0
    return l


def _from(moves, src):
    sd = O.label_srcdst()
    return {int(sd[m]) >> 8 for m in moves if (int(sd[m]) & 0xFF) == src[0] * 9 + src[1]}


def _sq(*yx):
    return {y * 9 + x for y, x in yx}


def test_rook_mate_in_the_palace():
    b = _pos(["r3K4", "8r", "9", "9", "9", "9", "9", "9", "9", "3k5"])
    assert len(O.legal_moves(b, 0)) == 3
    safe, flags = M.kingsafe(b, 0)
    assert len(safe) == 0 and flags == M.IN_CHECK | M.NO_SAFE_MOVE


def test_cannon_check_resolved_only_by_the_king_taking_the_screen():
    b = _pos(["4K4", "4n4", "9", "9", "9", "4c4", "9", "9", "9", "3rkr3"])
    assert len(O.legal_moves(b, 0)) == 3
    safe, flags = M.kingsafe(b, 0)
    assert list(safe) == [_label((0, 4), (1, 4))] and flags == M.IN_CHECK


def test_pinned_rook_moves_along_the_pin_only():
    b = _pos(["4K4", "9", "9", "4R4", "9", "9", "9", "9", "4r4", "3k5"])
    pseudo = O.legal_moves(b, 0)
    safe, flags = M.kingsafe(b, 0)
    assert _from(pseudo, (3, 4)) == _sq(*[(y, 4) for y in (1, 2, 4, 5, 6, 7, 8)], *[(3, x) for x in (0, 1, 2, 3, 5, 6, 7, 8)])
    assert _from(safe, (3, 4)) == _sq(*[(y, 4) for y in (1, 2, 4, 5, 6, 7, 8)])      # the capture of the pinning rook included
    assert flags == 0


def test_no_piece_may_become_the_screen_of_a_cannon():
    b = _pos(["4K4", "9", "9", "R8", "9", "9", "4c4", "9", "9", "3k5"])
    pseudo = O.legal_moves(b, 0)
    safe, flags = M.kingsafe(b, 0)
    assert flags == 0                                                                  # a cannon without a screen gives no check
    assert 3 * 9 + 4 in _from(pseudo, (3, 0))
    assert _from(safe, (3, 0)) == _from(pseudo, (3, 0)) - _sq((3, 4))


def test_knight_check_removed_by_blocking_the_leg():
    b = _pos(["4K4", "R8", "5n3", "9", "9", "9", "9", "9", "9", "3k5"])
    safe, flags = M.kingsafe(b, 0)
    assert flags & M.IN_CHECK and not flags & M.NO_SAFE_MOVE
    assert _from(safe, (1, 0)) == _sq((1, 5))                                          # the leg of (2, 5) -> (0, 4); every other rook move leaves the check
    assert _from(safe, (0, 4)) == _sq((0, 3), (1, 4), (0, 5)) - {q for q in _sq((0, 3), (1, 4), (0, 5)) if M.attacked(O.apply_move(b, _label((0, 4), divmod(q, 9)))[0], 0)}


def test_the_piece_between_the_kings_may_not_leave_the_file():
    b = _pos(["4K4", "9", "9", "9", "4R4", "9", "9", "9", "9", "4k4"])
    pseudo = O.legal_moves(b, 0)
    safe, flags = M.kingsafe(b, 0)
    assert len(_from(pseudo, (4, 4))) == 16
    assert _from(safe, (4, 4)) == _sq(*[(y, 4) for y in (1, 2, 3, 5, 6, 7, 8, 9)])     # taking the king is a move like any other
    assert flags == M.CAN_TAKE_KING


def test_stalemate_is_no_safe_move_without_check():
    b = _pos(["3K5", "8r", "9", "9", "9", "4r4", "9", "9", "9", "5k3"])
    assert len(O.legal_moves(b, 0)) == 2
    safe, flags = M.kingsafe(b, 0)
    assert len(safe) == 0 and flags == M.NO_SAFE_MOVE


def test_without_the_movers_king_every_move_is_king_safe():
    b = O.fen_to_board(O.START_FEN)
    b[4] = 0
    for side in (0, 1):
        safe, flags = M.kingsafe(b, side)
        if side == 0:
            assert np.array_equal(safe, O.legal_moves(b, 0)) and flags == 0
        else:
            assert flags & M.IN_CHECK == 0 and flags & M.CAN_TAKE_KING == 0


def test_flags_and_order_on_random_playouts():
    """bit 2 <=> the list is empty, and the king-safe list is a subsequence of the pseudo-legal one"""
    boards, side = M.playout_corpus(games=12, max_ply=120, seed=5)
    assert len(boards) > 800
    empties = 0
    for b, s in zip(boards, side):
        safe, flags = M.kingsafe(b, int(s))
        assert bool(flags & M.NO_SAFE_MOVE) == (len(safe) == 0)
        empties += len(safe) == 0
        it = iter(O.legal_moves(b, int(s)))
        assert all(any(m == p for p in it) for m in safe)
    assert empties >= 1
