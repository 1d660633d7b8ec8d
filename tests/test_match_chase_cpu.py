"""tests/match_model.py at the chase level (an evaluation match with the perpetual-chase rule, on the CPU oracle) against the figures it was
specified with: the 16-game fakenet match game by game, and the constructed chase played by search; and what the chase option
of the arena and of self-play refuses before any GPU is touched."""
import numpy as np
import pytest

import chase_cases as CC
import match_model as MM

# the 16-game match under the chase rule: reasons (chase = 9), plies and — sample_plies 0 — results for A
ROWS = {
    0: ([6, 3, 6, 9, 9, 6, 6, 6, 6, 9, 6, 9, 6, 9, 9, 9], [16, 160, 62, 29, 146, 34, 61, 60, 28, 97, 58, 57, 35, 30, 71, 123]),
    6: ([6, 9, 6, 9, 5, 6, 6, 9, 5, 5, 6, 6, 9, 9, 9, 9], [136, 15, 108, 117, 76, 49, 53, 64, 60, 94, 90, 81, 93, 30, 32, 74]),
}
RESULTS_0 = [0, 0, 0, 1, 1, 0, 0, 0, 0, -1, 0, -1, 0, 1, 1, 1]


@pytest.mark.parametrize("sample_plies", [0, 6])
def test_the_16_game_match_under_the_chase_rule(sample_plies):
    want = MM.fakenet_match(sample_plies)
    reasons, plies = ROWS[sample_plies]
    assert want["reason"].tolist() == reasons and want["plies"].tolist() == plies
    if sample_plies == 0:
        assert want["result"].tolist() == RESULTS_0
    chase, rep = want["reason"] == MM.CHASE, want["reason"] == MM.REPETITION
    assert chase.sum() >= 5 and rep.sum() >= 4
    assert (np.abs(want["result"][chase]) == 1).all() and (want["result"][rep] == 0).all()


def test_without_the_rule_the_chase_games_are_draws_by_repetition():
    on, off = MM.fakenet_match(0), MM.fakenet_match(0, chase=False)
    chase = on["reason"] == MM.CHASE
    assert chase.sum() == 7
    assert (off["reason"][chase] == MM.REPETITION).all() and (off["result"][chase] == 0).all()
    for k in ("plies", "moves", "a_red"):
        assert np.array_equal(on[k], off[k]), k
    for k in ("reason", "result"):
        assert np.array_equal(on[k][~chase], off[k][~chase]), k


def test_the_constructed_chase_played_by_search_is_lost_by_red_in_both_colour_assignments():
    f = (CC.steering_forward(), CC.CHASE_PLAYOUTS)
    line = [CC.label_of(m) for m in CC.CHASE_LINE]
    for game, result in ((0, -1), (1, 1)):           # game 0: A is red
        trace = []
        g = MM.play_game([f, f], CC.CHASE_BOARD, 0, 0, game, 64, rules="xiangqi", fold=3, chase=True, trace=trace)
        assert (g["reason"], g["result"], g["plies"], g["moves"]) == (MM.CHASE, result, 8, line)
        assert trace == [(8, 0, 2)]
        off = MM.play_game([f, f], CC.CHASE_BOARD, 0, 0, game, 64, rules="xiangqi", fold=3, chase=False)
        assert (off["reason"], off["result"], off["plies"], off["moves"]) == (MM.REPETITION, 0, 8, line)


def test_constants_and_what_the_options_refuse():
    from cchess_zero_amd import _lib, arena
    from cchess_zero_amd.selfplay import SelfPlay
    assert (_lib.MATCH_CHASE, _lib.CAUSE_NONE, _lib.CAUSE_CHECK, _lib.CAUSE_CHASE) == (MM.CHASE, 0, 1, 2)
    assert _lib.SP_CHASE_STATS == ("chases",) and arena.REASONS[9] == "chase" and 8 not in arena.REASONS
    assert arena.is_scored([7, 8, 9, 10]).tolist() == [True, False, True, False]
    for name in ("cz_threats", "cz_repetition_chase", "cz_match_set_chase", "cz_match_chase_history", "cz_selfplay_set_chase",
                 "cz_selfplay_chase_history", "cz_selfplay_chase_stats"):
        assert name in _lib.EXPORTS
    op = arena.Openings(CC.CHASE_BOARD[None], [0])
    f = (lambda planes: None, 4)
    with pytest.raises(ValueError, match="chase needs a repetition fold"):
        arena.Match(f, f, op, slots=2, rules="xiangqi", chase=True)
    with pytest.raises(ValueError, match="chase needs a repetition fold"):
        arena.Match(f, f, op, slots=2, chase=True)
    with pytest.raises(ValueError, match="repetition needs rules='xiangqi'"):
        arena.Match(f, f, op, slots=2, repetition=3, chase=True)
    m = arena.Match(f, f, op, slots=2, rules="xiangqi", repetition=3, chase=True)
    assert m.chase is True and arena.Match(f, f, op, slots=2, rules="xiangqi", repetition=3).chase is False
    with pytest.raises(ValueError, match="chase needs a repetition fold"):
        SelfPlay(None, None, 4, rules="xiangqi", chase=True)
    r = arena.MatchResult([1, 0, -1, 0], [1, 0, 1, 0], [8, 9, 10, 11], [9, 6, 9, 4], None, 0, 1.0, [], rules="xiangqi", repetition=3, chase=True)
    d = r.to_dict()
    assert (r.chases, r.repetitions, r.scored, r.wins, r.losses) == (2, 1, 3, 1, 1) and d["chase"] is True and d["chases"] == 2
    assert d["reasons"]["chase"] == 2
    plain = arena.MatchResult([0], [1], [8], [6], None, 0, 1.0, [], rules="xiangqi", repetition=3)
    assert plain.chase is False and plain.to_dict()["chases"] == 0
    with pytest.raises(SystemExit):
        arena.main(["--chase"])
