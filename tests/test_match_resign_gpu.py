"""Evaluation matches with resignation on the GPU (cz_match_set_resign, csrc/cz_match.hip) against tests/resign_model.py: the
16-game fixture match at threshold -0.125 on 6 slots — the queue refills, a resigned slot takes its next game — under king-capture
rules and under xiangqi + fold 3 + chase, every per-game array; and resignation off as the match was."""
import numpy as np
import pytest

import match_model as MM
import resign_model as R
from test_match_gpu import _fake_players

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("level", sorted(R.LEVELS))
def test_resigning_match_equals_the_model(level):
    from cchess_zero_amd.arena import Match
    lv = R.LEVELS[level]
    want = R.fakenet_match(-0.125, lv["rules"], lv["fold"], lv["chase"])
    n_resigned = int((want["reason"] == R.RESIGN).sum())
    print("model:", level, "reasons", want["reason"].tolist(), "plies", want["plies"].tolist(), "resigner", want["resigner"].tolist())
    assert n_resigned >= 4 and set(want["resigner"][want["reason"] == R.RESIGN].tolist()) == {0, 1} and n_resigned < 16
    res = Match(*_fake_players(), MM.fakenet_openings(), slots=6, max_plies=160, sample_plies=0, seed=5, nodes_per_tree=1 << 15,
                rules=lv["rules"], repetition=lv["fold"], chase=lv["chase"], resign=-0.125).play()
    MM.assert_equals_model(res, want, level)
    d = res.to_dict()
    assert res.resigns == n_resigned == d["reasons"]["resign"] == d["resigns"]
    assert res.aborted == 0 and res.scored == 16


def test_min_ply_holds_resignation_back_and_off_is_the_match_as_it_was():
    from cchess_zero_amd.arena import Match
    kw = dict(slots=6, max_plies=160, sample_plies=0, seed=5, nodes_per_tree=1 << 15)
    want = R.fakenet_match(-0.125, min_ply=20)
    assert (want["plies"][want["reason"] == R.RESIGN] >= 20).all() and (want["reason"] == R.RESIGN).sum() >= 4
    res = Match(*_fake_players(), MM.fakenet_openings(), resign=-0.125, resign_min_ply=20, **kw).play()
    MM.assert_equals_model(res, want, "min_ply")
    off = Match(*_fake_players(), MM.fakenet_openings(), **kw).play()
    MM.assert_equals_model(off, MM.fakenet_match(0, "capture", 0, False), "off")
    assert off.resigns == 0
