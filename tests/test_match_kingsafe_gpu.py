"""Evaluation matches under rules="xiangqi" (cz_match_set_rules(1): the move is chosen among the king-safe root children, a
mover without one is mated) against tests/match_model.py at the king-safe level, and rules="capture" against the match as it was."""
import numpy as np
import pytest

import kingsafe_model as KM
import match_model as MM
from test_match_gpu import _const_forward, _fake_players, _host_players, _one_opening

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def openings8():
    from cchess_zero_amd.arena import random_openings
    return random_openings(8, 4, seed=11)


def _board(rows):
    from oracle import oracle as O
    return O.fen_to_board("/".join(rows))


@pytest.mark.parametrize("sample_plies", [0, 6])
def test_xiangqi_match_equals_the_models_replay(openings8, sample_plies):
    from cchess_zero_amd.arena import Match
    want = MM.play_match(_host_players(), openings8, max_plies=160, sample_plies=sample_plies, seed=5, rules="xiangqi")
    for slots in (16, 6):   # 6 slots: the queue re-seeds slots as games end
        res = Match(*_fake_players(), openings8, slots=slots, max_plies=160, sample_plies=sample_plies, seed=5, nodes_per_tree=1 << 15,
                    rules="xiangqi").play()
        MM.assert_equals_model(res, want, slots)
        assert res.aborted == 0
        # a legal opening and king-safe moves only: no king is ever taken
        assert not (res.reason == MM.KING).any()
        assert res.rules == "xiangqi" and res.mates == int((want["reason"] == MM.MATE).sum()) == res.to_dict()["mates"]
        assert res.to_dict()["rules"] == "xiangqi" and res.to_dict()["reasons"]["mate"] == res.mates


def test_a_mated_root_loses_at_ply_0_in_both_colour_assignments():
    """Red to move: the king on e0 in check by the rook on a0, the rook on i1 guards rank 1 — three pseudo-legal king moves,
    none of them king-safe."""
    from oracle import oracle as O
    from cchess_zero_amd.arena import Match
    b = _board(["r3K4", "8r", "9", "9", "9", "9", "9", "9", "9", "3k5"])
    assert len(O.legal_moves(b, 0)) == 3 and KM.kingsafe(b, 0)[1] == KM.IN_CHECK | KM.NO_SAFE_MOVE
    f = (_const_forward(0.0), 6)
    res = Match(f, f, _one_opening(b, 0), slots=2, max_plies=8, rules="xiangqi").play()
    assert res.reason.tolist() == [MM.MATE, MM.MATE] and res.plies.tolist() == [0, 0]
    assert res.result.tolist() == [-1, 1]            # game 0: A is red and mated; game 1: B is red and mated
    assert res.moves == [[], []] and res.mates == 2 and res.scored == 2 and res.aborted == 0 and res.score == 0.5
    # under king-capture rules the same root is played on: red moves, and black takes the king
    res = Match(f, f, _one_opening(b, 0), slots=2, max_plies=8).play()
    assert res.plies.tolist()[0] >= 1 and res.mates == 0 and res.rules == "capture"


def test_the_most_visited_child_is_not_played_when_it_is_unsafe():
    """Red to move, kings on e0 / d9, red rook e3 pinned by the black rook e8.  The root's first child, king e0-d0, walks into
    the flying general; the root's U is 0 (quirk Q2), so a constant value of +0.5 sends one visit to every child and every
    further one to the first: the unsafe child has the most visits, and the king-safe maximum is played."""
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.arena import Match
    b = _board(["4K4", "9", "9", "4R4", "9", "9", "9", "9", "4r4", "3k5"])
    unsafe = int(tables()["lut"][4, 3])
    assert unsafe not in set(KM.kingsafe(b, 0)[0].tolist())
    f = (_const_forward(0.5, prefer=[unsafe]), 40)
    m = Match(f, f, _one_opening(b, 0), slots=2, max_plies=4, rules="xiangqi")
    m.start()
    m.search(0)
    m.search(1)
    N = [m.engines[p].root_stats_host() for p in (0, 1)]
    m.choose()
    played = m.played.cpu().numpy().view(np.uint16)
    safe = set(KM.kingsafe(b, 0)[0].tolist())
    for g, mover in ((0, 0), (1, 1)):   # game 0: A red moves, game 1: B red moves
        n = int(N[mover]["count"][g])
        vis, lab = N[mover]["N"][g, :n], N[mover]["label"][g, :n]
        top = int(np.argmax(vis))
        assert int(lab[top]) == unsafe and (vis[top] > np.delete(vis, top)).all()       # not vacuous: the unsafe child leads
        want = int(lab[MM.choose_safe(b, 0, lab, vis, 9, 0, 0, g)])
        assert int(played[g]) == want and want in safe and want != unsafe
        best_safe = max(int(v) for v, l in zip(vis, lab) if int(l) in safe)
        assert int(vis[list(lab).index(want)]) == best_safe
    m.close()
    # under king-capture rules the same search plays the unsafe move
    m = Match(f, f, _one_opening(b, 0), slots=2, max_plies=4)
    m.start(); m.search(0); m.search(1); m.choose()
    assert m.played.cpu().numpy().view(np.uint16).tolist() == [unsafe, unsafe]
    m.close()


def test_capture_rules_by_name_are_the_match_as_it_was(openings8):
    from cchess_zero_amd.arena import Match
    kw = dict(slots=6, max_plies=60, sample_plies=6, seed=5, nodes_per_tree=1 << 15)
    plain = Match(*_fake_players(), openings8, **kw)
    named = Match(*_fake_players(), openings8, rules="capture", **kw)
    rows = []
    for m in (plain, named):
        m.start()
        fin = 0
        while fin < m.n_games:
            for _ in range(8):
                m.step_ply()
            fin = m.finished()[0]
        rows.append(m.results())
        m.close()
    for k in ("result", "a_red", "plies", "reason", "moves"):
        assert np.array_equal(rows[0][k], rows[1][k]), k
    with pytest.raises(ValueError):
        Match(*_fake_players(), openings8, slots=2, rules="chess")
