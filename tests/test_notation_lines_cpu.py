"""Lines of moves in notation without a GPU: notation.line_text steps the board along a principal variation, and the UCCI
loop's `setoption Notation` writes the pv of its info lines with it while bestmove stays ICCS (the default is ICCS throughout)."""
import numpy as np

import notation_model as NM
from oracle import oracle as O
from test_ucci_cpu import _after, _library, _session  # noqa: F401  (the fixture builds the library)


def test_line_text_steps_the_board():
    from cchess_zero_amd.notation import START_FEN, fen_to_position, line_text
    b, s, _ = fen_to_position(START_FEN)
    l2i = {n: i for i, n in enumerate(O.labels())}
    line = [l2i[m] for m in "h2e2 h9g7 h0g2 i9h9 i0h0 g6g5 h0h6 b9c7".split()]
    assert line_text(b, s, line, "wxf") == "C2=5 H8+7 H2+3 R9=8 R1=2 P7+1 R2+6 H2+3".split()
    assert line_text(b, s, line, "chinese") == "炮二平五 馬8進7 馬二進三 車9平8 車一平二 卒7進1 車二進六 馬2進3".split()
    assert line_text(b, s, line, "iccs") == "h2e2 h9g7 h0g2 i9h9 i0h0 g6g5 h0h6 b9c7".split() and line_text(b, s, [], "wxf") == []
    assert np.array_equal(b, fen_to_position(START_FEN)[0])           # the caller's board is left alone


def test_ucci_info_lines_in_wxf():
    plain, _ = _session("position startpos moves h2e2\ngo nodes 48\nquit\n")
    wxf, eng = _session("setoption Notation wxf\nsetoption Notation xqf\nposition startpos moves h2e2\ngo nodes 48\nquit\n")
    assert eng.pv_notation == "wxf" and any(l.startswith("info string setoption Notation") and "xqf" in l for l in wxf)
    pv = lambda lines: [l for l in lines if l.startswith("info depth")][0].split("pv ")[1].split()
    assert [l for l in plain if l.startswith("bestmove")] == [l for l in wxf if l.startswith("bestmove")]
    # the WXF pv read back by the model from the position is the ICCS pv
    b, s, _ = _after("h2e2")
    import games_model as GM
    from cchess_zero_amd.notation import wxf_token
    got = []
    for t in pv(wxf):
        named = NM.Position(b, s, GM.legal_list(b, s, 0)).matching(wxf_token(t))
        assert len(named) == 1, t
        got.append(O.labels()[named[0]])
        b, s = O.apply_move(b, named[0])[0], s ^ 1
    assert got == pv(plain) and len(got) >= 1 and pv(wxf) != pv(plain)
