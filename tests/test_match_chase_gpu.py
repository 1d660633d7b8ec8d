"""Evaluation matches with the perpetual-chase rule (cz_match_set_chase: on a repeated position, a side that alone chased one
piece with every move of the cycle loses) against tests/match_model.py at the chase level, the third ring (cz_match_chase_history) against
Rules.threats, chase=False against the match as it was, and the setter's refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chase_cases as CC
import match_model as MM
from test_match_gpu import _fake_players, _one_opening

pytestmark = pytest.mark.gpu
KEYS = ("result", "a_red", "plies", "reason")


@functools.lru_cache(maxsize=None)
def _play(sample_plies, slots, chase):
    """One match per (sample_plies, slots, chase), shared by the tests below; read-only."""
    from cchess_zero_amd.arena import Match
    extra = dict(chase=True) if chase else {}
    return Match(*_fake_players(), MM.fakenet_openings(), slots=slots, max_plies=160, sample_plies=sample_plies, seed=5,
                 nodes_per_tree=1 << 15, rules="xiangqi", repetition=3, **extra).play()


# ---- 1. the model's replay -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [16, 6])        # 6 slots: the queue re-seeds slots as games end, the rings are not reset
@pytest.mark.parametrize("sample_plies", [0, 6])
def test_chase_match_equals_the_models_replay(sample_plies, slots):
    want = MM.fakenet_match(sample_plies)
    print("model: reasons", want["reason"].tolist(), "plies", want["plies"].tolist())
    assert int((want["reason"] == MM.CHASE).sum()) >= 5 and int((want["reason"] == MM.REPETITION).sum()) >= 4
    res = _play(sample_plies, slots, True)
    MM.assert_equals_model(res, want, (sample_plies, slots))
    assert res.aborted == 0
    d = res.to_dict()
    assert res.chase is True and d["chase"] is True
    assert res.chases == int((want["reason"] == MM.CHASE).sum()) == d["chases"] == d["reasons"]["chase"]
    assert res.repetitions == int((want["reason"] == MM.REPETITION).sum()) and res.perpetuals == int((want["reason"] == MM.PERPETUAL).sum())
    lost_by_a = (want["reason"] == MM.CHASE) & (want["result"] == -1)
    assert res.scored == 16 and res.losses >= int(lost_by_a.sum())


@pytest.mark.parametrize("sample_plies", [0, 6])
def test_against_the_same_match_without_the_rule_only_the_chase_games_differ(sample_plies):
    on, off = _play(sample_plies, 16, True), _play(sample_plies, 16, False)
    chase = on.reason == MM.CHASE
    assert chase.sum() >= 5 and off.chase is False and off.chases == 0
    assert (off.reason[chase] == MM.REPETITION).all() and (off.result[chase] == 0).all()
    assert np.array_equal(on.plies, off.plies) and np.array_equal(on.a_red, off.a_red) and on.moves == off.moves
    assert np.array_equal(on.reason[~chase], off.reason[~chase]) and np.array_equal(on.result[~chase], off.result[~chase])


# ---- 2. the constructed chase ------------------------------------------------------------------------------------------------
def test_the_constructed_chase_is_lost_by_red_in_both_colour_assignments():
    from cchess_zero_amd.arena import Match
    f = (CC.steering_device_forward(), CC.CHASE_PLAYOUTS)
    op = _one_opening(CC.CHASE_BOARD, 0)
    res = Match(f, f, op, slots=2, max_plies=64, rules="xiangqi", repetition=3, chase=True).play()
    assert res.reason.tolist() == [MM.CHASE, MM.CHASE] and res.plies.tolist() == [8, 8]
    assert res.result.tolist() == [-1, 1]            # red chases: game 0 has A red, game 1 B red
    assert res.moves == [CC.CHASE_LINE] * 2
    assert (res.chases, res.perpetuals, res.repetitions, res.scored, res.losses, res.wins, res.score) == (2, 0, 0, 2, 1, 1, 0.5)
    res = Match(f, f, op, slots=2, max_plies=64, rules="xiangqi", repetition=3).play()       # without the rule: a draw
    assert res.reason.tolist() == [MM.REPETITION] * 2 and res.result.tolist() == [0, 0] and res.moves == [CC.CHASE_LINE] * 2


# ---- 3. the ring -------------------------------------------------------------------------------------------------------------
def test_the_third_ring_holds_the_threats_of_every_root_position():
    from cchess_zero_amd.arena import Match
    from cchess_zero_amd.rules import Rules
    m = Match(*_fake_players(), MM.fakenet_openings(), slots=16, max_plies=160, seed=5, nodes_per_tree=1 << 15, rules="xiangqi",
              repetition=3, chase=True)
    m.start()
    rules = Rules()
    nonempty = 0
    for ply in range(10):
        m.search(0)
        m.search(1)
        act_a, act_b, game = m.active()
        roots = [m.engines[p].root_state() for p in (0, 1)]
        a = torch.from_numpy(act_a.astype(bool)).to(roots[0][0].device)
        board = torch.where(a[:, None], roots[0][0], roots[1][0])
        side = torch.where(a, roots[0][1], roots[1][1])
        want = rules.threats(board, side).cpu().numpy().view(np.uint64)
        m.choose()
        ring = m.chase_history()
        live = game == np.arange(16)
        assert live.sum() >= 12
        assert np.array_equal(ring[live, ply & 63], want[live]), ply
        nonempty += int(((want[live, 0] | want[live, 1]) != 0).sum())
        m.follow()
        m.adjudicate()
    m.close()
    assert nonempty >= 20


# ---- 4. off is off -----------------------------------------------------------------------------------------------------------
def test_chase_false_is_the_repetition_match_as_it_was():
    from cchess_zero_amd._lib import CchessHipError
    from cchess_zero_amd.arena import Match
    kw = dict(slots=6, max_plies=60, sample_plies=6, seed=5, nodes_per_tree=1 << 15, rules="xiangqi", repetition=3)
    rows = []
    for extra in ({}, dict(chase=False)):
        m = Match(*_fake_players(), MM.fakenet_openings(), **kw, **extra)
        m.start()
        fin = 0
        while fin < m.n_games:
            for _ in range(8):
                m.step_ply()
            fin = m.finished()[0]
        rows.append(m.results())
        with pytest.raises(CchessHipError, match="cz_match_set_chase first"):
            m.chase_history()
        m.close()
    for k in KEYS + ("moves",):        # per game; which slot a queued game runs in is not fixed, so the rings are not compared
        assert rows[0][k].tobytes() == rows[1][k].tobytes(), k
    assert not (rows[0]["reason"] == MM.CHASE).any() and (rows[0]["reason"] == MM.REPETITION).any()


# ---- 5. the switch -----------------------------------------------------------------------------------------------------------
def test_set_chase_refuses_what_it_cannot_keep():
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd.arena import Match
    L = lib()
    EINVAL = -1
    f = _fake_players(4, 3)
    m = Match(*f, _one_opening(CC.CHASE_BOARD, 0), slots=2, max_plies=8, rules="xiangqi")
    m.start()
    assert L.cz_match_set_chase(m._h, 1) == EINVAL and b"cz_match_set_repetition" in L.cz_last_error()      # needs a fold
    assert L.cz_match_chase_history(m._h, None) == EINVAL
    assert L.cz_match_set_chase(m._h, 0) == 0                                                # off stays off
    assert L.cz_match_set_repetition(m._h, 3) == 0
    for on in (2, -1):
        assert L.cz_match_set_chase(m._h, on) == EINVAL
    assert L.cz_match_set_chase(None, 1) == EINVAL
    assert L.cz_match_set_chase(m._h, 1) == 0
    assert L.cz_match_set_repetition(m._h, 0) == EINVAL and b"cz_match_set_chase(match, 0) first" in L.cz_last_error()
    assert L.cz_match_set_repetition(m._h, 2) == 0                                            # another fold is fine
    p = C.c_void_p()
    assert L.cz_match_chase_history(m._h, C.byref(p)) == 0 and p.value
    assert L.cz_match_set_chase(m._h, 0) == 0 and L.cz_match_set_repetition(m._h, 0) == 0
    assert L.cz_match_set_repetition(m._h, 3) == 0
    m.search(0)
    m.search(1)
    m.choose()
    assert L.cz_match_set_chase(m._h, 1) == EINVAL and b"before the first cz_match_choose" in L.cz_last_error()
    m.follow()
    m.adjudicate()
    m.close()
