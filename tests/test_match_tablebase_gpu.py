"""Tablebase adjudication in evaluation matches on the GPU (cz_match_set_tablebase, csrc/cz_match.hip; Match(tablebase=...)).
The oracle needs no second game loop: every finished game's recorded moves are replayed from its opening on the host
(tests/perft_model.py) and every position after a move is asked of tests/tablebase_set_model.py on the recorded tables — a game
ends at the first covered position after a move of its own, with the model's verdict, and nowhere else by a table."""
import numpy as np
import pytest

import match_model as MM
import perft_model as PM
import tablebase_model as TM
import tablebase_set_model as SM

pytestmark = pytest.mark.gpu
IN_SET = ["K-K", "KR-K", "K-KR"]


def _place(**pieces):
    b = np.zeros(90, np.uint8)
    for sq, code in pieces.items():
        b[9 * int(sq[1]) + "abcdefghi".index(sq[0])] = code
    return b


def _flip(board, side):
    """the position with the colours swapped: ranks reversed, red <-> black, the other side to move"""
    b = np.asarray(board, np.uint8).reshape(10, 9)[::-1].reshape(90)
    return np.where(b == 0, 0, np.where(b > 7, b - 7, b + 7)).astype(np.uint8), 1 - int(side)


def model_value(values, board, side):
    """IN_SET's answer from the recorded K-K and KR-K tables alone: K-KR is KR-K with the colours swapped"""
    v, _ = SM.probe(values, ["K-K", "KR-K"], board, side)
    if v == SM.MISS:
        v, _ = SM.probe(values, ["KR-K"], *_flip(board, side))
    return v


# all red to move.  The first three are covered themselves (one ply is played first): a win for red, a win for black, a draw;
# then positions a capture away from the set, and one that no capture brings into it
OPENINGS = [
    _place(d0=1, a4=3, e9=8),                    # KR-K
    _place(d0=1, a5=10, e9=8),                   # K-KR
    _place(d0=1, f9=8),                          # K-K
    _place(d0=1, a4=3, e9=8, a8=12),             # KR-KN: the knight hangs
    _place(e0=1, e1=10, f9=8),                   # K-KR, the rook en prise to the king: K-K after the capture, K-KR after a king step
    _place(d0=1, c2=5, d4=13, e9=8),             # KN-KP: KN-K is not in the set
    _place(d0=1, b2=5, h7=12, e9=8),             # KN-KN: never in the set
]


@pytest.fixture(scope="module")
def tb():
    from cchess_zero_amd.tablebase import Tablebase
    t = Tablebase()
    t.build("KR-K")
    t.build("K-KR")
    values, _ = TM.golden()
    assert np.array_equal(t.tables["KR-K"].cpu().numpy(), values["KR-K"]) and np.array_equal(t.tables["K-K"].cpu().numpy(), values["K-K"])
    return t


def _match(tablebase, **kw):
    from cchess_zero_amd.arena import Match, Openings
    op = Openings(np.stack(OPENINGS), np.zeros(len(OPENINGS), np.uint8))
    players = [(MM.device_forward("pos", 11), 12), (MM.device_forward("signed", 12), 8)]
    return Match(*players, op, slots=6, max_plies=6, rules="xiangqi", nodes_per_tree=1 << 12, tablebase=tablebase, **kw)


def test_games_end_where_the_model_says(tb):
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.arena import REASONS, is_scored
    l2i = tables()["label2i"]
    values, _ = TM.golden()
    dset = tb.device_set(IN_SET)
    try:
        m = _match(dset)
        res = m.play()
    finally:
        dset.close()                                  # Match.play has destroyed the match: nothing holds the set
    assert dset.h is None and res.unfinished == 0 and res.games == 2 * len(OPENINGS)
    by_tb, colours = 0, set()
    for g in range(res.games):
        b, side = OPENINGS[g // 2].copy(), 0
        covered_at = []
        for k, name in enumerate(res.moves[g]):
            b, _ = PM.make_move(b, int(l2i[name]))
            side ^= 1
            v = model_value(values, b, side)
            if SM.covered(v):
                covered_at.append((k, v))
        assert len(res.moves[g]) == int(res.plies[g])
        if int(res.reason[g]) == SM.TABLEBASE:
            # the first covered position after a move of the game is its last, and the result is the model's verdict for A
            assert len(covered_at) == 1 and covered_at[0][0] == len(res.moves[g]) - 1, (g, covered_at, res.moves[g])
            how, loser = SM.verdict(covered_at[0][1], side)
            assert how == SM.TABLEBASE and int(res.result[g]) == SM.result_for_a(loser, int(res.a_red[g])), (g, covered_at, loser)
            by_tb += 1
            colours.add({0: "black wins", 1: "red wins", -1: "draw"}[loser])
        else:
            assert not covered_at, (g, REASONS[int(res.reason[g])], covered_at, res.moves[g])
    print("reasons:", res.to_dict()["reasons"], "adjudicated:", sorted(colours))
    assert by_tb >= 6 and by_tb < res.games               # the three covered openings, both colour assignments; KN-KN never
    assert {"red wins", "black wins"} <= colours or "draw" in colours
    assert colours == {"red wins", "black wins", "draw"}   # openings 0, 1 and 2 end after their first ply
    assert res.tablebase is True and res.tablebases == by_tb == res.to_dict()["tablebases"] == res.to_dict()["reasons"]["tablebase"]
    assert res.scored == int(is_scored(res.reason, tablebase=True).sum()) and res.scored >= by_tb
    for g in (0, 1):                                      # KR-K: red has won after one ply, whoever plays red
        assert int(res.reason[g]) == SM.TABLEBASE and int(res.plies[g]) == 1 and int(res.result[g]) == (1 if res.a_red[g] else -1)
    for g in (12, 13):
        assert int(res.reason[g]) != SM.TABLEBASE


def test_without_a_set_no_game_carries_the_reason(tb):
    res = _match(None).play()
    assert res.unfinished == 0 and not (res.reason == SM.TABLEBASE).any() and res.tablebase is False and res.tablebases == 0


def test_setter_order(tb):
    from cchess_zero_amd._lib import CchessHipError, call
    dset = tb.device_set(IN_SET)
    m = _match(None)
    m.rules = "capture"
    m.start()
    try:
        with pytest.raises(CchessHipError, match=r"cz_match_set_tablebase: cz_match_set_rules\(match, 1\) first"):
            call("cz_match_set_tablebase", m._h, dset.h)
        call("cz_match_set_rules", m._h, 1)
        call("cz_match_set_tablebase", m._h, dset.h)
        with pytest.raises(CchessHipError, match=r"cz_match_set_rules: the table set needs rules 1: cz_match_set_tablebase\(match, NULL\) first"):
            call("cz_match_set_rules", m._h, 0)
        with pytest.raises(CchessHipError, match="cz_tb_set_destroy: the set is attached"):
            dset.close()
        m.step_ply()                                   # a set attached after the start judges from the next adjudicate on
        assert m.finished()[0] >= 6
    finally:
        m.close()                                      # cz_match_destroy gives the set back
        dset.close()
    assert dset.h is None
