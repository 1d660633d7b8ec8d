"""The repetition rule without a GPU: the model (tests/repetition_model.py) on hand-written histories, the arena's scoring of
the two new endings, Match's argument checks, and the constructed perpetual check replayed with the match model
(tests/match_model.py at the repetition level) on the CPU oracle."""
import numpy as np
import pytest

import match_model as MM
import repetition_cases as RC
import repetition_model as RM


# ---- 1. the model on hand-written histories ------------------------------------------------------------------------------
CYCLE = [1, 2, 3, 4, 1, 2, 3, 4, 1]        # position 8 is the third occurrence of position 0, red (0) to move in it


def _checks(n, at):
    c = [0] * n
    for i in at:
        c[i] = 1
    return c


def test_no_repetition_and_a_second_occurrence_under_fold_3():
    assert RM.verdict([1, 2, 3, 4, 5], [0] * 5, 0) == (RM.NONE, -1)
    assert RM.verdict([7], [1], 1) == (RM.NONE, -1)
    assert RM.verdict([1, 2, 3, 4, 1], [0] * 5, 0, fold=3) == (RM.NONE, -1)
    assert RM.verdict([1, 2, 3, 4, 1], [0] * 5, 0, fold=2) == (RM.DRAW, 0)


def test_a_third_occurrence_is_a_draw():
    assert RM.verdict(CYCLE, [0] * 9, 0) == (RM.DRAW, 0)
    assert RM.verdict(CYCLE, _checks(9, [1, 5, 6]), 0) == (RM.DRAW, 0)          # some checks, by both sides, none perpetual


def test_perpetual_check_by_red_by_black_and_by_both():
    black_to_move, red_to_move = [1, 3, 5, 7], [2, 4, 6, 8]                    # inside the cycle 1 .. 8, red to move at 8
    assert RM.verdict(CYCLE, _checks(9, black_to_move), 0) == (RM.RED_LOSES, 0)
    assert RM.verdict(CYCLE, _checks(9, red_to_move), 0) == (RM.BLACK_LOSES, 0)
    assert RM.verdict(CYCLE, _checks(9, black_to_move + red_to_move), 0) == (RM.DRAW, 0)
    assert RM.verdict(CYCLE, _checks(9, black_to_move[:-1]), 0) == (RM.DRAW, 0)  # red missed one check
    # the same history with black to move in the current position: the colours swap
    assert RM.verdict(CYCLE, _checks(9, black_to_move), 1) == (RM.BLACK_LOSES, 0)
    # position 0 is outside the cycle: its flag does not count
    assert RM.verdict(CYCLE, _checks(9, black_to_move + [0]), 0) == (RM.RED_LOSES, 0)


def test_the_window_must_reach_the_first_occurrence():
    assert RM.verdict(CYCLE, [0] * 9, 0, window=7) == (RM.NONE, -1)              # positions 1 .. 7: one earlier occurrence
    assert RM.verdict(CYCLE, [0] * 9, 0, window=8) == (RM.DRAW, 0)
    assert RM.verdict(CYCLE, [0] * 9, 0, window=100) == (RM.DRAW, 0)             # clamped to the history
    assert RM.verdict(CYCLE, [0] * 9, 0, window=0) == (RM.NONE, -1)
    assert RM.verdict(CYCLE, [0] * 9, 0, window=4, fold=2) == (RM.DRAW, 4)


def test_four_occurrences_under_fold_3_use_the_second_most_recent():
    keys = [1, 2, 1, 2, 1, 2, 1]                                                # 1 at 0, 2, 4 and, current, 6
    checks = _checks(7, [3, 5])                                                 # red's checks inside 3 .. 6; position 1 is none
    assert RM.verdict(keys, checks, 0, fold=3) == (RM.RED_LOSES, 2)
    assert RM.verdict(keys, checks, 0, fold=4) == (RM.DRAW, 0)                   # the longer cycle holds position 1
    assert RM.verdict(keys, checks, 0, fold=2) == (RM.RED_LOSES, 4)
    assert RM.verdict(keys, checks, 0, fold=5) == (RM.NONE, -1)


# ---- 2. the arena's scores -----------------------------------------------------------------------------------------------
def test_the_arena_scores_repetition_as_a_draw_and_perpetual_check_as_a_loss():
    from cchess_zero_amd import _lib, arena
    assert (_lib.MATCH_REPETITION, _lib.MATCH_PERPETUAL) == (6, 7) == (MM.REPETITION, MM.PERPETUAL)
    assert (_lib.REP_NONE, _lib.REP_DRAW, _lib.REP_RED_LOSES, _lib.REP_BLACK_LOSES) == (RM.NONE, RM.DRAW, RM.RED_LOSES, RM.BLACK_LOSES)
    assert arena.REASONS[6] == "repetition" and arena.REASONS[7] == "perpetual"
    assert arena.is_scored([0, 1, 2, 3, 4, 5, 6, 7, 8]).tolist() == [False, True, True, True, False, True, True, True, False]
    result = [-1, 1, 0, 0, 1, 0]
    reason = [7, 7, 6, 3, 1, 4]
    a_red = [1, 0, 1, 0, 1, 0]
    assert arena.pentanomial(result, reason).tolist() == [0, 0, 2, 0, 0]          # the pair with the aborted game is dropped
    res = arena.MatchResult(result, a_red, [8, 8, 30, 160, 50, 0], reason, None, 1000, 2.0, [], rules="xiangqi", repetition=3)
    assert (res.repetition, res.repetitions, res.perpetuals, res.mates, res.aborted, res.scored) == (3, 1, 2, 0, 1, 5)
    assert (res.wins, res.draws, res.losses) == (2, 2, 1)                        # the perpetual games are decisive: one lost, one won
    assert res.by_colour == {"red": dict(W=1, D=1, L=1), "black": dict(W=1, D=1, L=0)}
    assert res.score == pytest.approx(3.0 / 5.0)
    d = res.to_dict()
    assert d["reasons"]["repetition"] == 1 and d["reasons"]["perpetual"] == 2 and d["reasons"]["aborted"] == 1
    assert (d["repetition"], d["repetitions"], d["perpetuals"], d["rules"]) == (3, 1, 2, "xiangqi")
    plain = arena.MatchResult(result[3:5], a_red[3:5], [160, 50], reason[3:5], None, 10, 1.0, [])
    assert (plain.repetition, plain.repetitions, plain.perpetuals) == (0, 0, 0) and plain.to_dict()["repetition"] == 0


def test_match_refuses_a_repetition_rule_it_cannot_play():
    from cchess_zero_amd.arena import Match, Openings
    op = Openings(RC.perpetual_board()[None], [0])
    f = (lambda planes: None, 4)
    for kw in (dict(rules="capture", repetition=3), dict(repetition=3), dict(rules="xiangqi", repetition=1),
               dict(rules="xiangqi", repetition=9), dict(rules="xiangqi", repetition=-3)):
        with pytest.raises(ValueError):
            Match(f, f, op, slots=2, **kw)
    m = Match(f, f, op, slots=2, rules="xiangqi", repetition=3)                   # no GPU work before start()
    assert m.repetition == 3 and Match(f, f, op, slots=2, rules="xiangqi").repetition == 0


# ---- 3. the constructed perpetual check on the CPU oracle --------------------------------------------------------------
@pytest.mark.parametrize("playouts", [24, RC.PERPETUAL_PLAYOUTS, 40])
def test_the_constructed_perpetual_check_is_lost_by_the_checking_side(playouts):
    from oracle import oracle as O
    import kingsafe_model as KM
    b = RC.perpetual_board()
    lab = O.labels()
    after = RC.perpetual_checked_positions()
    assert all(KM.attacked(p, 1) and not KM.attacked(p, 0) for p in after) and not KM.attacked(b, 0) and not KM.attacked(b, 1)
    players = [(RC.steering_forward(), playouts)] * 2
    want_moves = RC.PERPETUAL_LINE * 2
    for game, result in ((0, -1), (1, 1)):       # game 0: A is red, the checking side; game 1: B is red
        trace = []
        g = MM.play_game(players, b, 0, 0, game, 64, rules="xiangqi", fold=3, trace=trace)
        assert (g["reason"], g["plies"], g["result"], g["a_red"]) == (MM.PERPETUAL, 8, result, 1 - game)
        assert [lab[m] for m in g["moves"]] == want_moves
        assert trace == [(8, 0)]                 # the third occurrence at ply 8, the cycle starts from the opening
    # with the rule off the same players walk the loop on
    g = MM.play_game(players, b, 0, 0, 0, 24, rules="xiangqi", fold=0)
    assert g["reason"] not in (MM.REPETITION, MM.PERPETUAL) and g["plies"] > 8
