"""Analyzer.analyse(history=) and Analyzer.repetition on the GPU: the moves the repetition rule bans in the positions of the
constructed lines, against tests/repmoves_model.py; without a history nothing changes."""
import numpy as np
import pytest

import chase_cases as CC
import repetition_cases as RC
import repmoves_model as M
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def test_analyse_reports_the_banned_moves_of_the_constructed_lines():
    from cchess_zero_amd.analysis import Analyzer
    from cchess_zero_amd.net import PolicyValueNet
    an = Analyzer(PolicyValueNet(res_block_nums=1, seed=3), 16, 4)
    boards, sides, _ = CC.play_line(RC.perpetual_board(), 0, RC.PERPETUAL_LINE * 2)
    cb, cs, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE * 2)
    game = lambda b, s, n: [(b[i], int(s[i]), i) for i in range(n + 1)]
    pos = [game(boards, sides, 6)[-1], game(boards, sides, 7)[-1], game(cb, cs, 6)[-1], game(boards, sides, 3)[-1]]
    hist = [game(boards, sides, 6)[:-1], game(boards, sides, 7)[:-1], game(cb, cs, 6)[:-1], None]
    plain = an.analyse(pos)
    got = an.analyse(pos, history=hist, repetition=3, chase=True)
    assert all("repetition" not in r for r in plain)
    assert [{k: v for k, v in r.items() if k != "repetition"} for r in got] == plain
    rep = [r["repetition"] for r in got]
    assert rep[3] is None and all(r["fold"] == 3 and r["chase"] and not r["forced"] for r in rep[:3])
    assert rep[0]["banned"] == [dict(move="d5e5", verdict="reply", cause="check", reply="e9d9")] and rep[0]["wins"] == []
    assert rep[1]["banned"] == [] and rep[1]["wins"] == [dict(move="e9d9", cause="check")]
    assert rep[2]["banned"] == [dict(move="a6a5", verdict="reply", cause="chase", reply="b5b6")]
    # the same from the model, move by move
    L = O.labels()
    for p, h, r in zip(pos[:3], hist[:3], rep[:3]):
        g = h + [p]
        keys, checks, recs = M.history_of([q[0] for q in g], [q[1] for q in g])
        m = M.repetition_moves(p[0], p[1], keys, checks, recs, p[2], 3)
        assert [b["move"] for b in r["banned"]] == [L[x] for x, l in zip(m["moves"], m["losing"]) if l]
    # without the chase rule the chase is a draw: nothing banned; fold 2 bans one cycle earlier
    assert an.repetition(pos[2:3], hist[2:3], 3, False)[0]["banned"] == []
    two = an.repetition([game(boards, sides, 2)[-1]], [game(boards, sides, 2)[:-1]], 2)[0]
    assert [b["move"] for b in two["banned"]] == ["d5e5"]
    # the line from the start position by its moves, as the command line does it
    line = an.play((RC.perpetual_board(), 0, 0), RC.PERPETUAL_LINE + RC.PERPETUAL_LINE[:2])
    assert len(line) == 7 and np.array_equal(line[-1][0], boards[6]) and line[-1][1:] == (0, 6)
    with pytest.raises(ValueError):
        an.play((RC.perpetual_board(), 0, 0), ["e5d5", "d9d8"])
