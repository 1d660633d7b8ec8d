"""tests/chase_model.py (the specification of the perpetual-chase rule) against the expected values it was written from: the
table of threatened sets, the constructed chase ply by ply in both colours, the order of check and chase, and a count of how
often every exclusion clause fires."""
import numpy as np
import pytest

import chase_cases as CC
import chase_model as CM
from kingsafe_model import playout_corpus


@pytest.mark.parametrize("name,board,side,want", CC.TABLE, ids=[c[0] for c in CC.TABLE])
def test_table(name, board, side, want):
    assert CM.threats(board, side) == want
    assert [CM.mirror_sq(q) for q in CM.threats(CM.mirror(board), 1 - side)] == want      # the other colour


@pytest.mark.parametrize("mirrored", [False, True])
def test_constructed_chase_ply_by_ply(mirrored):
    boards, sides, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE, mirrored)
    keys, chk, recs = CC.history(boards, sides)
    assert not chk.any()
    for i, want in enumerate(CC.CHASE_THREATS):
        got = CM.threats(boards[i], int(sides[i]))
        assert (sorted(CM.mirror_sq(q) for q in got) if mirrored else got) == want, i
        own = int(recs[i][2]) | (int(recs[i][3]) << 64)
        assert own == CM.bits(np.nonzero((boards[i] >= 8) if sides[i] else ((boards[i] >= 1) & (boards[i] <= 7)))[0])
    for n in range(len(boards)):
        v = CM.verdict(keys[:n + 1].tolist(), chk[:n + 1].tolist(), recs[:n + 1], int(sides[n]), None, 3)
        if n < 8:
            assert v == (CM.NONE, -1, CM.CAUSE_NONE), (n, v)
        else:       # the chaser (red; black in the mirrored game) loses
            assert v == (CM.BLACK_LOSES if mirrored else CM.RED_LOSES, 0, CM.CAUSE_CHASE), v
    assert CM.verdict(keys.tolist(), chk.tolist(), recs, int(sides[8]), None, 2) == (CM.BLACK_LOSES if mirrored else CM.RED_LOSES, 4, CM.CAUSE_CHASE)


def test_a_window_shorter_than_the_cycle_is_no_verdict():
    boards, sides, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE)
    keys, chk, recs = CC.history(boards, sides)
    assert CM.verdict(keys.tolist(), chk.tolist(), recs, 0, 7, 3) == (CM.NONE, -1, CM.CAUSE_NONE)
    assert CM.verdict(keys.tolist(), chk.tolist(), recs, 0, 8, 3)[0] == CM.RED_LOSES
    assert CM.verdict(keys.tolist(), chk.tolist(), recs, 0, 3, 2) == (CM.NONE, -1, CM.CAUSE_NONE)
    assert CM.verdict(keys.tolist(), chk.tolist(), recs, 0, 0, 3) == (CM.NONE, -1, CM.CAUSE_NONE)


def test_check_outranks_chase_and_two_chasers_draw():
    # the current position (8) is even with side_now to move: the even positions follow the moves of 1 - side_now
    for side_now in (0, 1):
        loses = lambda x: CM.RED_LOSES if x == 0 else CM.BLACK_LOSES
        k, c, r = CC.synthetic_cycle(True, False)
        assert CM.verdict(k, c, r, side_now) == (loses(1 - side_now), 0, CM.CAUSE_CHASE)
        k, c, r = CC.synthetic_cycle(False, True)
        assert CM.verdict(k, c, r, side_now) == (loses(side_now), 0, CM.CAUSE_CHASE)
        k, c, r = CC.synthetic_cycle(True, True)
        assert CM.verdict(k, c, r, side_now) == (CM.DRAW, 0, CM.CAUSE_NONE)               # both chase
        k, c, r = CC.synthetic_cycle(False, False)
        assert CM.verdict(k, c, r, side_now) == (CM.DRAW, 0, CM.CAUSE_NONE)               # neither does
        k, c, r = CC.synthetic_cycle(True, False, check_odd=1)                            # one side chases, the other checks: the checker loses
        assert CM.verdict(k, c, r, side_now) == (loses(side_now), 0, CM.CAUSE_CHECK)
        k, c, r = CC.synthetic_cycle(True, False, check_even=1, check_odd=1)              # both check: a draw whatever is chased
        assert CM.verdict(k, c, r, side_now) == (CM.DRAW, 0, CM.CAUSE_NONE)
        k, c, r = CC.synthetic_cycle(True, False, check_even=1)                           # the chaser checks too: cause check
        assert CM.verdict(k, c, r, side_now) == (loses(1 - side_now), 0, CM.CAUSE_CHECK)


def test_a_threat_must_follow_one_piece():
    k, c, r = CC.synthetic_cycle(True, False)
    r[4][0] = 1 << 0                                    # position 4 threatens another piece than the standing one
    assert CM.verdict(k, c, r, 0) == (CM.DRAW, 0, CM.CAUSE_NONE)
    k, c, r = CC.synthetic_cycle(True, False)
    for i in (2, 4, 6, 8):                              # the threatened piece is the one that moves: followed from square to square
        r[i][0] = 1 << ((i >> 1) & 1)
    assert CM.verdict(k, c, r, 0)[2] == CM.CAUSE_CHASE
    r[6][2] |= 1 << 33                                  # an occupancy that changes in another way than one move forgets everything
    assert CM.verdict(k, c, r, 0) == (CM.DRAW, 0, CM.CAUSE_NONE)


def test_corpus_shares_and_every_clause_fires():
    boards, side = playout_corpus(games=12, seed=2024)
    assert len(boards) == 1294
    reasons = {}
    sets = [CM.threats(b, int(s), reasons) for b, s in zip(boards, side)]
    assert sum(1 for t in sets if t) == 651 and max(len(t) for t in sets) == 3
    for name, b, s, _ in CC.TABLE:
        CM.threats(b, s, reasons)
    print("captures by clause:", sorted(reasons.items()))
    assert all(reasons.get(c, 0) >= 1 for c in (0, 1, 2, 3, 4, 5)), reasons
