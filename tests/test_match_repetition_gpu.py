"""Evaluation matches with the repetition rule (cz_match_set_repetition: a fold-th occurrence of a position ends the game, a
draw or a loss for the side that checked perpetually) against tests/match_model.py at the repetition level, the ring of positions
(cz_match_history) against the rules kernels, and repetition=0 against the match as it was."""
import ctypes as C

import numpy as np
import pytest
import torch

import match_model as MM
import repetition_cases as RC
from test_match_gpu import _fake_players, _one_opening

pytestmark = pytest.mark.gpu


def _play(sample_plies, slots, fold):
    from cchess_zero_amd.arena import Match
    return Match(*_fake_players(), MM.fakenet_openings(), slots=slots, max_plies=160, sample_plies=sample_plies, seed=5,
                 nodes_per_tree=1 << 15, rules="xiangqi", repetition=fold).play()


def _assert_equals_model(res, want, tag):
    MM.assert_equals_model(res, want, tag)
    assert res.aborted == 0


# ---- 1. the model's replay ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slots", [16, 6])        # 6 slots: the queue re-seeds slots as games end, the rings are not reset
@pytest.mark.parametrize("sample_plies", [0, 6])
def test_repetition_match_equals_the_models_replay(sample_plies, slots):
    want = MM.fakenet_match(sample_plies, fold=3, chase=False)
    print("model: reasons", np.bincount(want["reason"], minlength=8).tolist(), "plies", want["plies"].tolist())
    assert int((want["reason"] == MM.REPETITION).sum()) >= 12          # the rule decides most games: the comparison is not vacuous
    assert int((want["reason"] != MM.REPETITION).sum()) >= 1           # and the ply cap or a mate ends the others
    res = _play(sample_plies, slots, 3)
    _assert_equals_model(res, want, (sample_plies, slots))
    d = res.to_dict()
    assert res.repetition == 3 and res.repetitions == int((want["reason"] == MM.REPETITION).sum()) == d["reasons"]["repetition"]
    assert res.perpetuals == int((want["reason"] == MM.PERPETUAL).sum()) == d["perpetuals"] and d["repetition"] == 3


def test_twofold_repetition_ends_every_repeating_game_earlier():
    want2, want3 = MM.fakenet_match(0, fold=2, chase=False), MM.fakenet_match(0, fold=3, chase=False)
    rep2 = want2["reason"] == MM.REPETITION
    assert int(rep2.sum()) >= 12 and (want2["plies"][rep2] < want3["plies"][rep2]).all()
    _assert_equals_model(_play(0, 6, 2), want2, "fold 2")


# ---- 2. the constructed perpetual check ----------------------------------------------------------------------------------
def test_perpetual_check_loses_in_both_colour_assignments():
    from cchess_zero_amd.arena import Match
    f = (RC.steering_device_forward(), RC.PERPETUAL_PLAYOUTS)
    op = _one_opening(RC.perpetual_board(), 0)
    res = Match(f, f, op, slots=2, max_plies=64, rules="xiangqi", repetition=3).play()
    assert res.reason.tolist() == [MM.PERPETUAL, MM.PERPETUAL] and res.plies.tolist() == [8, 8]
    assert res.result.tolist() == [-1, 1]            # red checks with every move: game 0 has A red, game 1 B red
    assert res.moves == [RC.PERPETUAL_LINE * 2] * 2
    assert (res.perpetuals, res.repetitions, res.scored, res.losses, res.wins, res.score) == (2, 0, 2, 1, 1, 0.5)
    # without the rule the same players walk the loop on
    res = Match(f, f, op, slots=2, max_plies=24, rules="xiangqi").play()
    assert not np.isin(res.reason, (MM.REPETITION, MM.PERPETUAL)).any() and (res.plies > 8).all()
    assert res.repetition == 0 and res.perpetuals == 0


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------
def test_the_ring_holds_the_movers_root_position_of_every_ply():
    from cchess_zero_amd.arena import Match
    from cchess_zero_amd.rules import Rules
    m = Match(*_fake_players(), MM.fakenet_openings(), slots=16, max_plies=160, seed=5, nodes_per_tree=1 << 15, rules="xiangqi",
              repetition=3)
    m.start()
    rules = Rules()
    for ply in range(10):
        m.search(0)
        m.search(1)
        act_a, act_b, game = m.active()
        roots = [m.engines[p].root_state() for p in (0, 1)]
        a = torch.from_numpy(act_a.astype(bool)).to(roots[0][0].device)
        board = torch.where(a[:, None], roots[0][0], roots[1][0])
        side = torch.where(a, roots[0][1], roots[1][1])
        want_key = rules.hash(board, side).cpu().numpy().view(np.uint64)
        want_check = rules.in_check(board, side).cpu().numpy() & 1
        m.choose()
        keys, checks = m.history()
        live = game == np.arange(16)                 # 16 slots for 16 games: a slot plays its first game or is parked
        assert live.sum() >= 12 and ((act_a | act_b) == live).all()
        assert np.array_equal(keys[live, ply & 63], want_key[live]), ply
        assert np.array_equal(checks[live, ply & 63], want_check[live]), ply
        m.follow()
        m.adjudicate()
    m.close()


# ---- 4. off is off -----------------------------------------------------------------------------------------------------
def test_repetition_0_is_the_xiangqi_match_as_it_was():
    from cchess_zero_amd.arena import Match
    kw = dict(slots=6, max_plies=60, sample_plies=6, seed=5, nodes_per_tree=1 << 15, rules="xiangqi")
    rows = []
    for extra in ({}, dict(repetition=0)):
        m = Match(*_fake_players(), MM.fakenet_openings(), **kw, **extra)
        m.start()
        fin = 0
        while fin < m.n_games:
            for _ in range(8):
                m.step_ply()
            fin = m.finished()[0]
        rows.append(m.results())
        if extra:
            from cchess_zero_amd._lib import CchessHipError
            with pytest.raises(CchessHipError, match="cz_match_set_repetition first"):
                m.history()
        m.close()
    for k in ("result", "a_red", "plies", "reason", "moves"):
        assert np.array_equal(rows[0][k], rows[1][k]), k
    assert not np.isin(rows[0]["reason"], (MM.REPETITION, MM.PERPETUAL)).any()


# ---- 5. the switch -------------------------------------------------------------------------------------------------------
def test_set_repetition_refuses_what_it_cannot_keep():
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd.arena import Match
    L = lib()
    EINVAL = -1
    f = _fake_players(4, 3)
    m = Match(*f, _one_opening(RC.perpetual_board(), 0), slots=2, max_plies=8)         # rules 0
    m.start()
    assert L.cz_match_set_repetition(m._h, 3) == EINVAL                                  # needs rules 1
    assert L.cz_match_history(m._h, None, None) == EINVAL
    assert L.cz_match_set_rules(m._h, 1) == 0
    for fold in (1, 9, -1):
        assert L.cz_match_set_repetition(m._h, fold) == EINVAL
    assert L.cz_match_set_repetition(None, 3) == EINVAL
    assert L.cz_match_set_repetition(m._h, 3) == 0 and L.cz_match_set_repetition(m._h, 0) == 0 and L.cz_match_set_repetition(m._h, 8) == 0
    assert L.cz_match_set_rules(m._h, 0) == EINVAL                                       # not while the fold is set
    pk, pc = C.c_void_p(), C.c_void_p()
    assert L.cz_match_history(m._h, C.byref(pk), C.byref(pc)) == 0 and pk.value and pc.value
    assert L.cz_match_set_repetition(m._h, 0) == 0 and L.cz_match_set_rules(m._h, 0) == 0 and L.cz_match_set_rules(m._h, 1) == 0
    m.close()
    m = Match(*f, _one_opening(RC.perpetual_board(), 0), slots=2, max_plies=8, rules="xiangqi")
    m.start()
    m.search(0)
    m.search(1)
    m.choose()
    assert L.cz_match_set_repetition(m._h, 3) == EINVAL                                  # a history from mid-game would be wrong
    assert L.cz_last_error()
    m.follow()
    m.adjudicate()
    m.close()
