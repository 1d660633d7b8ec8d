"""--avoid_repetition / avoid_repetition=: the option checks (cchess_zero_amd.rules), and the model's window cap.  No GPU."""
import argparse

import pytest

import repetition_cases as RC
import repmoves_model as M


def test_avoid_needs_a_repetition_fold():
    from cchess_zero_amd.rules import add_rule_flags, check_rule_flags, check_rule_options
    with pytest.raises(ValueError, match="Match: avoid_repetition needs a repetition fold"):
        check_rule_options("Match", "xiangqi", 0, False, avoid=True)
    check_rule_options("Match", "xiangqi", 3, False, avoid=True)
    check_rule_options("Match", "capture", 0, False, avoid=False)
    ap = argparse.ArgumentParser()
    add_rule_flags(ap, "the games")
    assert ap.parse_args([]).avoid_repetition is False
    check_rule_flags(ap, ap.parse_args(["--rules", "xiangqi", "--repetition", "3", "--chase", "--avoid_repetition"]), "arena")
    with pytest.raises(SystemExit):
        check_rule_flags(ap, ap.parse_args(["--rules", "xiangqi", "--avoid_repetition"]), "arena")


def test_the_window_cap_of_a_ring_cuts_what_lies_63_plies_back():
    """The constructed line with 60 made-up plies behind its first position: the reply to d5e5 makes position 64, equal to
    position 0.  Uncapped, fold 2 sees the reply complete the repetition; with the ring's cap of 63 the reply's window
    (min(w + 2, 63)) does not reach position 0."""
    import chase_cases as CC
    boards, sides, _ = CC.play_line(RC.perpetual_board(), 0, RC.PERPETUAL_LINE)
    keys, checks, _ = M.history_of(boards, sides, chase=False)
    k = keys[:1] + [50000 + i for i in range(60)] + keys[1:3]
    c = checks[:1] + [(i & 1) ^ 1 for i in range(60)] + checks[1:3]
    free = M.repetition_moves(boards[2], 0, k, c, None, None, 2)
    capped = M.repetition_moves(boards[2], 0, k, c, None, 63, 2, wcap=63)
    assert free["summary"] == M.REMOVED and capped["summary"] == 0 and len(capped["allowed"]) == len(free["allowed"]) + 1
