"""WXF and Chinese move notation without a GPU: tests/notation_model.py (the rule by which a token names a move, restated from
include/cchess_hip.h) against hand-written anchors, the writer (cchess_zero_amd/notation.py: move_text — from the notations'
rules, no matcher in it) against the model in a round trip over EVERY listed move of every position of the reference's six
games and of the corpus at both rule levels, the spellings the readers accept, and parse_games / write_games with notations."""
import numpy as np
import pytest

import games_model as GM
import notation_cases as NC
import notation_model as NM
from oracle import oracle as O


def l2i():
    return {s: i for i, s in enumerate(O.labels())}


def play(board, side, texts, read, rules=1):
    """texts read by `read` and named by the model, one after the other -> the label strings"""
    out, board, side = [], np.array(board, np.uint8), int(side)
    for t in texts:
        named = NM.Position(board, side, GM.legal_list(board, side, rules)).matching(read(t))
        assert len(named) == 1, (t, named)
        out.append(O.labels()[named[0]])
        board, side = O.apply_move(board, named[0])[0], side ^ 1
    return out


def test_anchors_from_the_opening():
    from cchess_zero_amd.notation import chinese_token, wxf_token
    want = "h2e2 h9g7 h0g2 i9h9 i0h0 g6g5 h0h6 b9c7".split()
    assert play(GM.start_board(), 0, "C2=5 H8+7 H2+3 R9=8 R1=2 P7+1 R2+6 H2+3".split(), wxf_token) == want
    assert play(GM.start_board(), 0, "炮二平五 馬8進7 馬二進三 車9平8 車一平二 卒7進1 車二進六 馬2進3".split(), chinese_token) == want


def test_anchors_with_two_cannons_on_a_file():
    from cchess_zero_amd.notation import chinese_token, fen_to_position, move_text, wxf_token
    b, s, _ = fen_to_position("3k5/9/9/9/9/9/9/4C4/4C4/5K3 w")
    for text, zh, move in (("C+=4", "前炮平四", "e2f2"), ("C-=6", "後炮平六", "e1d1"), ("C++1", "前炮進一", "e2e3")):
        assert play(b, s, [text], wxf_token) == [move] and play(b, s, [zh], chinese_token) == [move]
        assert move_text(b, s, l2i()[move], "wxf") == text and move_text(b, s, l2i()[move], "chinese") == zh and move_text(b, s, l2i()[move], "iccs") == move


def test_a_file_digit_names_every_piece_of_the_kind_on_the_file():
    """the digit form is not the writer's for two cannons on a file, but a text may use it: it names both"""
    from cchess_zero_amd.notation import fen_to_position, wxf_token
    b, s, _ = fen_to_position("3k5/9/9/9/9/9/9/4C4/4C4/5K3 w")
    p = NM.Position(b, s, GM.legal_list(b, s, 1))
    assert sorted(p.matching(wxf_token("C5=4"))) == sorted([l2i()["e2f2"], l2i()["e1f1"]])
    assert p.matching(wxf_token("C5+1")) == [l2i()["e2e3"]] and p.matching(wxf_token("C5-1")) == [l2i()["e1e0"]]


def _positions():
    """every position of the six reference games and of the corpus (as far as the model made them), once"""
    c = NC.corpus()
    seen, out = set(), []
    for g in range(NC.G):
        b, s = c["boards"][g].copy(), int(c["side"][g])
        labels = c["model"][0]["labels_out"][g]
        for i in range(int(c["model"][0]["valid"][g]) + 1):
            key = (b.tobytes(), s)
            if key not in seen and not GM.refused(b, s):
                seen.add(key)
                out.append((b.copy(), s))
            if i < int(c["model"][0]["valid"][g]):
                b, s = O.apply_move(b, int(labels[i]))[0], s ^ 1
    return out


def test_round_trip_of_every_listed_move():
    """a condition, not a statistic: the writer has a text for every move of every list (the material is standard), in WXF and
    in Chinese, both read to one token, and the model reads that token back to exactly that move — at both rule levels"""
    from cchess_zero_amd.notation import chinese_token, move_text, move_token, wxf_token
    positions = _positions()
    assert len(positions) > 1000
    moves = forms = 0
    for b, s in positions:
        for rules in (0, 1):
            lst = GM.legal_list(b, s, rules)
            p = NM.Position(b, s, lst)
            for m in (int(x) for x in lst):
                w, z = move_text(b, s, m, "wxf"), move_text(b, s, m, "chinese")
                assert w is not None and z is not None, (b, s, m)
                t = wxf_token(w)
                assert t == chinese_token(z) == move_token(b, s, m), (w, z)
                assert p.matching(t) == [m], (O.labels()[m], w, z, [O.labels()[x] for x in p.matching(t)])
                moves += 1
                forms += w[1] in "+-abcde"
    print("round trip: %d positions, %d moves, %d in an ordinal form" % (len(positions), moves, forms))
    assert moves > 50000 and forms > 500


def test_the_writer_has_no_text_for_three_of_a_kind():
    from cchess_zero_amd.notation import fen_to_position, move_text
    b, s, _ = fen_to_position("3k5/9/9/9/9/R8/R8/R8/9/5K3 w")
    assert move_text(b, s, l2i()["a3b3"], "wxf") is None and move_text(b, s, l2i()["a3b3"], "chinese") is None
    assert move_text(b, s, l2i()["a3b3"], "iccs") == "a3b3" and move_text(b, s, l2i()["f0f1"], "wxf") == "K4+1"
    with pytest.raises(ValueError):
        move_text(b, s, l2i()["a3b3"], "pgn")


def test_pawn_forms_of_the_writer():
    from cchess_zero_amd.notation import fen_to_position, move_text
    five, _, _ = fen_to_position(NC.P5_FEN + " w")
    assert [move_text(five, 0, l2i()[m], "wxf") for m in ("c8b8", "c7b7", "c6b6", "c5b5")] == ["P+=8", "Pb=8", "Pc=8", "Pd=8"]
    assert [move_text(five, 0, l2i()[m], "chinese") for m in ("c8b8", "c7b7", "c6b6", "c5b5")] == ["前兵平八", "二兵平八", "三兵平八", "四兵平八"]
    three, _, _ = fen_to_position(NC.BP3_FEN + " b")
    assert [move_text(three, 1, l2i()[m], "chinese") for m in ("g2h2", "g3f3", "g4h4")] == ["前卒平8", "中卒平6", "後卒平8"]
    two, _, _ = fen_to_position(NC.P22_FEN + " w")
    assert [move_text(two, 0, l2i()[m], "wxf") for m in ("c6d6", "e6d6", "c5b5")] == ["7+=6", "5+=6", "7-=8"]
    assert [move_text(two, 0, l2i()[m], "chinese") for m in ("c6d6", "e5f5")] == ["前七平六", "後五平四"]


def test_every_accepted_spelling_is_one_token():
    from cchess_zero_amd.notation import chinese_token, token_text, wxf_token
    for spellings, canon in ((("H2+3", "N2+3", "h2+3", "n2+3"), "H2+3"), (("E3+5", "B3+5", "b3+5", "e3+5"), "E3+5"), (("C2=5", "C2.5", "c2.5"), "C2=5"),
                             (("R+=4", "+R=4", "+r.4", "r+.4"), "R+=4"), (("P-+1", "-P+1"), "P-+1"), (("Pb=4", "PB=4", "pb.4"), "Pb=4"),
                             (("7+=6", "+7=6", "7+.6"), "7+=6"), (("A4+5", "a4+5"), "A4+5"), (("K5-1", "k5-1"), "K5-1")):
        assert {token_text(wxf_token(s)) for s in spellings} == {canon}, spellings
    for spellings, canon in ((("帥五進一", "帅五进一", "將5進1", "将５进１"), "K5+1"), (("仕四退五", "士4退5"), "A4-5"), (("相三進五", "象3进5"), "E3+5"),
                             (("傌二進三", "馬二進三", "马2进3"), "H2+3"), (("俥一平二", "車一平二", "车1平2"), "R1=2"),
                             (("炮二平五", "砲二平五", "包2平5"), "C2=5"), (("兵七進一", "卒7进1"), "P7+1"),
                             (("前炮退二", "前砲退2"), "C+-2"), (("後車平四", "后车平4"), "R-=4"), (("中兵平四", "二兵平四", "2卒平4"), "Pb=4"),
                             (("三兵進一",), "Pc+1"), (("前三平四", "前3平4"), "3+=4"), (("後七進一", "后七进一"), "7-+1"), (("二七平六",), "7b=6")):
        assert {token_text(chinese_token(s)) for s in spellings} == {canon}, spellings
    for bad in ("", "C2=", "C2=55", "X2=5", "C0=5", "C2=0", "C2*5", "Cf=5", "22=5", "h2e2", "炮二平五", None, 5):
        with pytest.raises(ValueError) as e:
            wxf_token(bad)
        assert repr(bad) in str(e.value)
    for bad in ("", "炮二平", "炮二飛五", "龍二平五", "炮十平五", "六兵平四", "前前平四", "C2=5", None):
        with pytest.raises(ValueError) as e:
            chinese_token(bad)
        assert repr(bad) in str(e.value)


def test_parse_games_with_notations():
    from cchess_zero_amd import games as GG
    from cchess_zero_amd.notation import wxf_token
    tok = lambda s: tuple(wxf_token(t) for t in s.split())
    lines = "C2=5 H8+7 1-0\nh2e2 h9g7 0-1\n炮二平五 馬8進7 1/2-1/2\nC2=5 h9g7 1-0\nC2=5 Z8+7\n炮二平五 H8+7\n"
    g = GG.parse_games(lines, notations=GG.NOTATIONS)
    assert [x.tokens for x in g] == [tok("C2=5 H8+7"), None, tok("C2=5 H8+7")] and [x.result for x in g] == [1, -1, 0]
    assert g[1].labels == (l2i()["h2e2"], l2i()["h9g7"]) and g[0].labels == () and [s[0] for s in g.skipped] == [4, 5, 6]
    assert "h9g7" in g.skipped[0][1] and "Z8+7" in g.skipped[1][1] and "H8+7" in g.skipped[2][1]      # mixed, wrong, mixed: the text is named
    # the default reads what it always read, and says so as it always did
    d = GG.parse_games(lines)
    assert len(d) == 1 and d[0].labels == g[1].labels and d[0].tokens is None and [s[0] for s in d.skipped] == [1, 3, 4, 5, 6]
    assert all("is not an ICCS move" in s[1] for s in d.skipped)
    assert GG.Game(b"", 0, 0, (), None, ()).tokens is None
    pgn = ('[Format "WXF"]\n[Result "1-0"]\n1. C2=5 H8+7 2. +R=4 1-0\n\n'         # the tag decides
           '[Format "Chinese"]\n[Result "*"]\n1. 炮二平五 馬8進7\n\n'
           '[Result "0-1"]\n1. C2.5 n8+7 0-1\n\n'                                 # no tag: the first move decides
           '[Format "WXF"]\n[Result "1-0"]\n1. h2e2 1-0\n\n'                      # the tag says WXF, the text is not
           '[Format "XQF"]\n[Result "1-0"]\n1. C2=5 1-0\n\n'
           '[Result "1-0"]\n1. H2-E2 H8+7 1-0\n')                                 # ICCS first, then WXF
    p = GG.parse_games(pgn, notations=GG.NOTATIONS)
    assert [x.tokens for x in p] == [tok("C2=5 H8+7 R+=4"), tok("C2=5 H8+7"), tok("C2=5 H8+7")] and len(p.skipped) == 3
    why = " | ".join(s[1] for s in p.skipped)
    assert "'h2e2'" in why and "XQF" in why and "'H8+7'" in why
    only = GG.parse_games(pgn, notations=("iccs", "wxf"))
    assert [x.tokens for x in only] == [tok("C2=5 H8+7 R+=4"), tok("C2=5 H8+7")] and "Chinese" in " ".join(s[1] for s in only.skipped)
    assert len(GG.parse_games(pgn)) == 0 and len(GG.parse_games(pgn).skipped) == 6
    with pytest.raises(ValueError):
        GG.parse_games(pgn, notations=("wxf", "xqf"))


class _Replay:
    """what write_games reads of a GameReplayer.replay answer, from the model's records"""

    def __init__(self, per_game, kept):
        recs = [g["records"][:g["valid"]] for g, k in zip(per_game, kept) if k]
        self.records = np.concatenate(recs)
        self.game_of_record = np.repeat(np.nonzero(kept)[0], [len(r) for r in recs]).astype(np.int32)


def test_write_games_in_notation_and_back():
    from cchess_zero_amd import games as GG
    moves, lens, results, _, _ = GM.golden_games()
    gs = GG.games_from_labels(moves, lens, results)
    m = GM.replay(None, None, moves, lens, results, 0)
    kept = np.array([True, True, False, True, True, True])              # game 2 did not come back from the replay
    for notation, tag in (("wxf", "WXF"), ("chinese", "Chinese")):
        text = GG.write_games(gs, notation=notation, replay=_Replay(m["per_game"], kept))
        assert text.count('[Format "%s"]' % tag) == 5 and text.count('[Format "ICCS"]') == 1
        back = GG.parse_games(text, notations=GG.NOTATIONS)
        assert len(back) == 6 and back.skipped == () and back[2] == gs[2]
        c = NC.corpus()
        for g in (0, 1, 3, 4, 5):                                       # the corpus holds these very games as the writer's tokens
            assert back[g].tokens == tuple(int(t) for t in c["tokens"][g, :lens[g]]) and back[g].labels == () and back[g].result == gs[g].result
        # a game of tokens goes out as WXF without a replay, and as ICCS with one
        assert GG.parse_games(GG.write_games(back), notations=GG.NOTATIONS) == back
        iccs = GG.parse_games(GG.write_games(back, replay=_Replay(m["per_game"], np.ones(6, bool))))
        assert list(iccs) == gs
    with pytest.raises(ValueError):
        GG.write_games(gs, notation="wxf")
