"""Matches with the avoid step (cz_match_set_avoid, Match(avoid_repetition=True)): the games equal tests/avoid_model.py's replay
of tests/match_model.py's loop bit for bit, the constructed perpetual check is no longer lost at ply 8, off is the match as it
was, and the setter keeps its order."""
import numpy as np
import pytest

import avoid_model as AM
import match_model as MM
import repetition_cases as RC
from test_match_gpu import _fake_players, _host_players, _one_opening

pytestmark = pytest.mark.gpu
EINVAL = -1


def _model(sample_plies, chase, openings=None, players=None, max_plies=160):
    with AM.avoiding() as counters:
        want = MM.play_match(players or _host_players(), openings or MM.fakenet_openings(), max_plies, sample_plies, 5, None, "xiangqi", 3, chase)
    return want, counters


def test_avoid_match_equals_the_models_replay():
    """The first four opening pairs of the fixture match (8 games on 6 slots: the queue re-seeds slots) at the chase level: without
    the step three of them are lost by perpetual chase."""
    from cchess_zero_amd.arena import Match
    op = MM.fakenet_openings().subset(np.arange(4))
    want, counters = _model(0, True, op)
    plain = MM.play_match(_host_players(), op, 160, 0, 5, None, "xiangqi", 3, True)
    print("model: avoided %d forced %d; reasons with the step %s, without %s" % (counters["avoided"], counters["forced_repetitions"],
          np.bincount(want["reason"], minlength=12).tolist(), np.bincount(plain["reason"], minlength=12).tolist()))
    assert counters["avoided"] >= 1 and not np.array_equal(want["moves"], plain["moves"])          # the step acts on this match
    assert int((plain["reason"] == MM.CHASE).sum()) >= 1 and int((want["reason"] == MM.CHASE).sum()) < int((plain["reason"] == MM.CHASE).sum())
    kw = dict(slots=6, max_plies=160, sample_plies=0, seed=5, nodes_per_tree=1 << 15, rules="xiangqi", repetition=3, chase=True)
    res = Match(*_fake_players(), op, avoid_repetition=True, **kw).play()
    MM.assert_equals_model(res, want, "avoid")
    d = res.to_dict()
    assert (res.avoided, res.forced_repetitions) == (counters["avoided"], counters["forced_repetitions"]) == (d["avoided"], d["forced_repetitions"])
    # off: the match as it was, and its summary has no new key
    off = Match(*_fake_players(), op, **kw).play()
    MM.assert_equals_model(off, plain, "off")
    assert "avoided" not in off.to_dict() and (off.avoided, off.forced_repetitions) == (0, 0)


def test_the_constructed_perpetual_check_is_no_longer_lost_at_ply_8():
    from cchess_zero_amd.arena import Match
    f = (RC.steering_device_forward(), RC.PERPETUAL_PLAYOUTS)
    hf = (RC.steering_forward(), RC.PERPETUAL_PLAYOUTS)
    op = _one_opening(RC.perpetual_board(), 0)
    off = Match(f, f, op, slots=2, max_plies=24, rules="xiangqi", repetition=3).play()
    assert off.reason.tolist() == [MM.PERPETUAL] * 2 and off.plies.tolist() == [8, 8] and off.result.tolist() == [-1, 1]     # red loses at ply 8
    res = Match(f, f, op, slots=2, max_plies=24, rules="xiangqi", repetition=3, avoid_repetition=True).play()
    want, counters = _model(0, False, op, [hf, hf], 24)
    MM.assert_equals_model(res, want, "constructed")
    assert res.avoided >= 1 and res.avoided == counters["avoided"]
    for g in range(2):
        assert not (res.reason[g] == MM.PERPETUAL and res.plies[g] == 8)
        assert res.moves[g][:6] == (RC.PERPETUAL_LINE * 2)[:6] and res.moves[g][6] != "d5e5"      # red leaves the line at its last chance


def test_set_avoid_keeps_the_setters_order():
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd.arena import Match
    L = lib()
    m = Match(*_fake_players(4, 3), _one_opening(RC.perpetual_board(), 0), slots=2, max_plies=8, rules="xiangqi")
    m.start()
    assert L.cz_match_set_avoid(None, 1) == EINVAL and L.cz_match_avoid_stats(None, None, None) == EINVAL
    assert L.cz_match_set_avoid(m._h, 1) == EINVAL                       # needs a fold
    assert L.cz_match_set_repetition(m._h, 3) == 0 and L.cz_match_set_avoid(m._h, 2) == EINVAL and L.cz_match_set_avoid(m._h, 1) == 0
    assert L.cz_match_set_repetition(m._h, 0) == EINVAL                  # not while the step is on
    assert L.cz_match_set_avoid(m._h, 0) == 0 and L.cz_match_set_repetition(m._h, 0) == 0 and L.cz_match_set_repetition(m._h, 3) == 0
    assert m.avoid_stats() == (0, 0)
    m.search(0)
    m.search(1)
    m.choose()
    assert L.cz_match_set_avoid(m._h, 1) == EINVAL and b"before the first cz_match_choose" in L.cz_last_error()
    m.follow()
    m.adjudicate()
    m.close()
