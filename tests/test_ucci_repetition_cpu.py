"""The UCCI engine's own repetition rule (setoption Repetition / Chase): the stand-in searcher of tests/test_ucci_cpu.py, its
repetition_moves answered by tests/repmoves_model.py on the history the engine hands over.  No GPU."""
import numpy as np
import pytest

import chase_cases as CC
import repetition_cases as RC
import repmoves_model as M
from test_ucci_cpu import OracleSearcher, _session

FEN = "3k5/9/9/9/4R4/9/9/9/9/5K3 w"      # repetition_cases.perpetual_board: red K f0, R e5, black k d9, red to move
LINE = "e5d5 d9e9 d5e5 e9d9 e5d5 d9e9"


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__
    __graft_entry__.build_hip_only()


class RepetitionSearcher(OracleSearcher):
    """OracleSearcher with the model's repetition_moves; asked: what the engine handed over"""

    def __init__(self):
        super().__init__()
        self.asked = []

    def repetition_moves(self, boards, sides, window, fold, chase):
        self.asked.append((len(boards), int(window), fold, chase))
        keys, checks, recs = M.history_of(boards, sides, chase)
        r = M.repetition_moves(boards[-1], int(sides[-1]), keys, checks, recs, window, fold)
        return dict(moves=np.array(r["moves"], np.uint16), verdict=np.array(r["verdict"], np.uint8), reply=np.array(r["reply"], np.uint16),
                    reply_verdict=np.array(r["reply_verdict"], np.uint8), allowed=M.KM.mask_of(r["allowed"]), summary=r["summary"])


def best(lines):
    return [l.split()[1] for l in lines if l.startswith("bestmove")]


def test_fen_is_the_constructed_board():
    from cchess_zero_amd.notation import fen_to_position
    b, s, rr = fen_to_position(FEN)
    assert np.array_equal(b, RC.perpetual_board()) and (s, rr) == (0, 0)


def test_the_checker_is_kept_from_the_losing_move_and_the_other_side_takes_the_win():
    s = RepetitionSearcher()
    lines, eng = _session("setoption Repetition 3\nposition fen %s moves %s\ngo nodes 40\nquit\n" % (FEN, LINE), s)
    assert "info string repetition: banned d5e5" in lines and best(lines) and best(lines)[0] != "d5e5"
    assert s.asked == [(7, 6, 3, False)] and len(eng.history) == 7 and eng.ban == []
    assert lines.index("info string repetition: banned d5e5") < min(i for i, l in enumerate(lines) if l.startswith("info depth"))
    # whatever the search would like: every number of playouts answers another move
    for nodes in (1, 8, 90):
        lines, _ = _session("setoption Repetition 3\nposition fen %s moves %s\ngo nodes %d\nquit\n" % (FEN, LINE, nodes), RepetitionSearcher())
        assert best(lines)[0] != "d5e5"
    # one ply later black plays e9d9 at once: no search
    s = RepetitionSearcher()
    lines, _ = _session("setoption Repetition 3\nposition fen %s moves %s d5e5\ngo nodes 40\nquit\n" % (FEN, LINE), s)
    assert best(lines) == ["e9d9"] and s.resets == 0
    assert "info string repetition: e9d9 ends the game, the opponent checked perpetually" in lines
    info = [l for l in lines if l.startswith("info depth")]
    assert len(info) == 1 and info[0].split()[:7] == ["info", "depth", "1", "score", "29999", "nodes", "0"] and info[0].endswith("pv e9d9")
    # a GUI's ban on that move is respected: the engine searches
    s = RepetitionSearcher()
    lines, _ = _session("setoption Repetition 3\nposition fen %s moves %s d5e5\nbanmoves e9d9\ngo nodes 40\nquit\n" % (FEN, LINE), s)
    assert best(lines) == [] and "nobestmove" in lines                    # e9d9 is black's only king-safe move


def test_chase_option_and_fold():
    line = " ".join(CC.CHASE_LINE[:6])
    fen = "4k4/9/9/1c7/R8/9/9/9/9/3K5 w"
    from cchess_zero_amd.notation import fen_to_position
    assert np.array_equal(fen_to_position(fen)[0], CC.CHASE_BOARD)
    lines, _ = _session("setoption Repetition 3\nposition fen %s moves %s\ngo nodes 30\nquit\n" % (fen, line), RepetitionSearcher())
    assert not any(l.startswith("info string repetition") for l in lines)           # without the chase rule the cycle is a draw
    s = RepetitionSearcher()
    lines, _ = _session("setoption Repetition 3\nsetoption Chase true\nposition fen %s moves %s\ngo nodes 30\nquit\n" % (fen, line), s)
    assert "info string repetition: banned a6a5" in lines and best(lines)[0] != "a6a5" and s.asked == [(7, 6, 3, True)]
    lines, _ = _session("setoption Repetition 3\nsetoption Chase true\nposition fen %s moves %s a6a5\ngo nodes 30\nquit\n" % (fen, line), RepetitionSearcher())
    assert best(lines) == ["b5b6"] and "info string repetition: b5b6 ends the game, the opponent chased perpetually" in lines
    # fold 2 sees it one cycle earlier; a halfmove clock in the FEN cuts nothing off the engine's own history
    lines, _ = _session("setoption Repetition 2\nposition fen %s - - 0 1 moves %s\ngo nodes 30\nquit\n" % (FEN, "e5d5 d9e9"), RepetitionSearcher())
    assert "info string repetition: banned d5e5" in lines
    lines, eng = _session("setoption Repetition 9\nsetoption Repetition x\nsetoption Chase maybe\nquit\n")
    assert eng.repetition == 0 and eng.chase is False and len([l for l in lines if l.startswith("info string setoption")]) == 3


def test_every_move_loses_is_said_and_searched():
    c = M.forced_case()

    class Forced(RepetitionSearcher):
        def repetition_moves(self, boards, sides, window, fold, chase):
            r = M.model_of(c)
            return dict(moves=np.array(r["moves"], np.uint16), verdict=np.array(r["verdict"], np.uint8), reply=np.array(r["reply"], np.uint16),
                        reply_verdict=np.array(r["reply_verdict"], np.uint8), allowed=M.KM.mask_of(r["allowed"]), summary=r["summary"])
    from cchess_zero_amd.notation import position_to_fen
    lines, _ = _session("setoption Repetition 2\nposition fen %s\ngo nodes 20\nquit\n" % position_to_fen(c["board"], 0), Forced())
    assert "info string repetition: every move loses" in lines and best(lines) == ["e2c0"]


def test_gui_bans_on_every_move_that_does_not_lose_leave_the_losing_move():
    safe = [M.O.labels()[m] for m in M.KM.kingsafe(RC.perpetual_board(), 0)[0]]      # position 6 is the start board with the rook on d5
    import chase_cases as CC
    boards, sides, _ = CC.play_line(RC.perpetual_board(), 0, LINE.split())
    others = [M.O.labels()[m] for m in M.KM.kingsafe(boards[6], 0)[0] if M.O.labels()[m] != "d5e5"]
    lines, _ = _session("setoption Repetition 3\nposition fen %s moves %s\nbanmoves %s\ngo nodes 20\nquit\n" % (FEN, LINE, " ".join(others)),
                        RepetitionSearcher())
    assert "info string repetition: every move loses" in lines and best(lines) == ["d5e5"] and safe


def test_repetition_off_is_todays_transcript_and_an_illegal_move_keeps_the_history():
    script = "ucci\nisready\nposition fen %s moves %s\ngo nodes 40\nposition startpos moves h2e2\nbanmoves h9g7\ngo nodes 24\nquit\n" % (FEN, LINE)
    plain = OracleSearcher()                               # a searcher without repetition_moves: the option off never asks for it
    off, _ = _session(script, plain, clock=lambda: 0.0)        # a clock that stands: the time fields are equal too
    zero, _ = _session("setoption Repetition 0\nsetoption Chase false\n" + script, RepetitionSearcher(), clock=lambda: 0.0)
    assert off == zero and not any("repetition" in l for l in off)
    # the parent's engine answers d5e5 or not, as its search likes; the transcript above is the one it writes: no new line
    assert [l.split()[0] for l in off if l.startswith(("info", "bestmove"))] == ["info", "bestmove", "info", "bestmove"]
    s = RepetitionSearcher()
    lines, eng = _session("setoption Repetition 3\nposition fen %s moves %s\nposition fen %s moves e5d5 d9d8\ngo nodes 40\nquit\n" % (FEN, LINE, FEN), s)
    assert any(l.startswith("info string illegal move d9d8") for l in lines)
    assert len(eng.history) == 7 and s.asked == [(7, 6, 3, False)] and "info string repetition: banned d5e5" in lines
