"""Resignation on the CPU: suggest_resign_threshold against a brute-force count, the play-on draw, tests/resign_model.py's match
on the 16-game fixture against the values a replay on the CPU oracle gave when the feature was specified, MatchResult with the
new reason, and the self-play fixture's mix of endings (which the GPU tests of tests/test_selfplay_resign_gpu.py replay)."""
import numpy as np
import pytest

import match_model as MM
import resign_model as R


# ---- suggest_resign_threshold ----------------------------------------------------------------------------------------------------
def _hists():
    rng = np.random.default_rng(7)
    one = np.zeros(64, np.int64)
    one[29] = 500
    ends = np.zeros(64, np.int64)
    ends[0], ends[63] = 150, 50
    return dict(empty=np.zeros(64, np.int64), few=np.bincount([3, 40, 40], minlength=64), one=one, ends=ends,
                spread=rng.integers(0, 40, 64), sparse=np.where(rng.random(64) < 0.2, rng.integers(1, 300, 64), 0))


@pytest.mark.parametrize("name", sorted(_hists()))
def test_suggest_resign_threshold_equals_the_brute_force_count(name):
    from cchess_zero_amd.selfplay import suggest_resign_threshold
    hist = _hists()[name]
    for target in (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 1.0):
        for min_samples in (100, 1):
            got, want = suggest_resign_threshold(hist, target, min_samples), R.suggest_brute(hist, target, min_samples)
            assert got == want, (name, target, min_samples, got, want)
            if got is not None:      # the definition, stated directly: the share of entries below the edge, and no larger edge holds it
                b = round((got + 1.0) * 32)
                assert got == -1.0 + b / 32.0 and hist[:b].sum() / hist.sum() <= target
                assert b == 64 or hist[:b + 1].sum() / hist.sum() > target


def test_suggest_resign_threshold_on_the_hand_made_cases():
    from cchess_zero_amd.selfplay import suggest_resign_threshold
    h = _hists()
    assert suggest_resign_threshold(h["empty"], 0.05) is None and suggest_resign_threshold(h["empty"], 1.0, min_samples=0) is None
    assert suggest_resign_threshold(h["few"], 0.05) is None                      # 3 entries < min_samples
    assert suggest_resign_threshold(h["few"], 0.05, min_samples=3) == -1.0 + 3 / 32.0
    # all mass in bin 29 = [-0.09375, -0.0625): any target below 1 stops at the bin's lower edge, target 1 takes everything
    assert suggest_resign_threshold(h["one"], 0.0) == suggest_resign_threshold(h["one"], 0.99) == -1.0 + 29 / 32.0
    assert suggest_resign_threshold(h["one"], 1.0) == 1.0
    # target 0 with an entry in bin 0: the only edge with nothing below it is -1 (nobody ever resigns)
    assert suggest_resign_threshold(h["ends"], 0.0) == -1.0
    assert suggest_resign_threshold(h["ends"], 0.75) == -1.0 + 63 / 32.0 and suggest_resign_threshold(h["ends"], 0.74) == -1.0


# ---- the play-on draw --------------------------------------------------------------------------------------------------------------
def test_the_play_on_draw_is_the_matchs_construction_and_fair():
    for seed, slot, game_no in ((0, 0, 0), (5, 3, 9), (148, 7, 2), ((1 << 64) - 1, 8191, (1 << 32) - 1)):
        h = MM.splitmix64(seed ^ MM.splitmix64((slot << 32) | game_no))
        assert R.uniform(seed, slot, game_no) == (h >> 11) * 2.0 ** -53
    # match_model.uniform is the same construction over (game << 16) | ply: the same counter gives the same number
    assert R.uniform(5, 0, 3 << 16 | 7) == MM.uniform(5, 3, 7)
    u = np.array([R.uniform(148, slot, game_no) for slot in range(64) for game_no in range(64)])
    assert len(u) == 4096 and ((0.0 <= u) & (u < 1.0)).all() and len(set(u.tolist())) == 4096
    assert abs((u < 0.25).mean() - 0.25) <= 0.03, (u < 0.25).mean()


# ---- the match on the 16-game fixture ------------------------------------------------------------------------------------------------
RESIGNED_125 = {1: (34, 0), 2: (34, 0), 4: (7, 1), 6: (1, 1), 7: (18, 0), 8: (2, 0), 9: (78, 0), 11: (6, 0), 13: (18, 0), 15: (28, 0)}
RESIGNED_1875 = {7: (42, 0), 8: (15, 1), 9: (78, 0), 11: (6, 0), 13: (18, 0)}      # game: (ply, the side that resigns, 0 = red)


@pytest.mark.parametrize("threshold,resigned", [(-0.125, RESIGNED_125), (-0.1875, RESIGNED_1875)])
def test_the_fixture_match_resigns_where_the_replay_did(threshold, resigned):
    base = MM.fakenet_match(0, "capture", 0, False)
    got = R.fakenet_match(threshold)
    print("plies", got["plies"].tolist(), "reasons", got["reason"].tolist(), "resigner", got["resigner"].tolist())
    assert {g: (int(got["plies"][g]), int(got["resigner"][g])) for g in range(16) if got["reason"][g] == R.RESIGN} == resigned
    for g in range(16):
        if g in resigned:
            ply, side = resigned[g]
            a_moves = (side == 0) == bool(got["a_red"][g])                       # the resigner is A
            assert got["result"][g] == (-1 if a_moves else 1)
            assert np.array_equal(got["moves"][g, :ply], base["moves"][g, :ply]) and (got["moves"][g, ply:] == 0xFFFF).all()
            assert ply < base["plies"][g] and ply % 2 == side                    # every opening has red to move at an even ply
        else:                                                                    # row for row what the fixture gives without resignation
            for k in ("result", "a_red", "plies", "reason", "moves"):
                assert np.array_equal(got[k][g], base[k][g]), (g, k)
    assert (MM.fakenet_openings().side == 0).all()


def test_at_minus_01875_game_8_is_resigned_by_the_side_that_wins_it_played_out():
    base, got = MM.fakenet_match(0, "capture", 0, False), R.fakenet_match(-0.1875)
    assert got["reason"][8] == R.RESIGN and got["resigner"][8] == 1 and got["a_red"][8] == 1 and got["result"][8] == 1
    assert base["reason"][8] == MM.KING and base["result"][8] == -1              # played out, black (B) wins: a false positive


def test_match_result_knows_the_reason():
    from cchess_zero_amd import _lib, arena
    assert _lib.MATCH_RESIGN == 10 == R.RESIGN and arena.REASONS[10] == "resign" and 8 not in arena.REASONS
    assert _lib.SP_RESIGN_STATS == R.STATS
    reason = np.array([10, 1, 10, 4, 2, 10], np.uint8)
    result = np.array([1, -1, -1, 0, 0, 1], np.int8)
    # a match played with resignation scores its resigned games; without it the code counts as little as an unassigned one
    assert arena.is_scored(reason, resign=True).tolist() == [True, True, True, False, True, True] and not arena.is_scored([8], resign=True)[0]
    assert arena.is_scored(reason).tolist() == [False, True, False, False, True, False]
    r = arena.MatchResult(result, [1, 0] * 3, [3, 9, 4, 0, 60, 5], reason, None, 10, 1.0, [], resign=-0.125)
    assert (r.resigns, r.scored, r.aborted, r.wins, r.losses, r.draws, r.resign) == (3, 5, 1, 2, 2, 1, -0.125)
    # pairs: (resign +1, king -1) = 1 point of 2; (resign, aborted) dropped; (rr60 0, resign +1) = 1.5 points
    assert r.pentanomial.tolist() == [0, 0, 1, 1, 0]
    assert arena.MatchResult(result, [1, 0] * 3, [3, 9, 4, 0, 60, 5], reason, None, 10, 1.0, []).scored == 2
    d = r.to_dict()
    assert d["resigns"] == 3 == d["reasons"]["resign"] and d["reasons"]["king"] == 1 and d["resign"] == -0.125
    plain = arena.MatchResult([1], [1], [9], [1], None, 1, 1.0, [])
    assert plain.resigns == 0 and plain.to_dict()["resigns"] == 0 and plain.resign is None and plain.to_dict()["resign"] is None


# ---- the self-play fixture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", sorted(R.LEVELS))
def test_the_selfplay_fixture_holds_every_kind_of_game(level):
    """The model alone, under tests/resign_model.SP (threshold -0.125, 30 % play on, seed 148), 48 lock-step plies of 8 re-seeded slots:
      capture: 12 games, 3 resigned (1 by red, 2 by black), 4 play-on games finished: 1 crossed and lost, 1 crossed and did not lose
               (the false positive), 7 games ended the old way with no crossing;
      xiangqi + fold 3 + chase: 11 games, 5 resigned (2 by red, 3 by black), 3 play-on games finished: 1 crossed and lost, 2 false
               positives, 3 games ended the old way with no crossing."""
    out = R.sp_model(level)
    mix = R.sp_mix(out)
    print(level, mix, out["stats"], out["resign_stats"], {i: int(v) for i, v in enumerate(out["hist"]) if v}, "margin %.3g" % out["min_margin"])
    assert mix["resigned"] >= 2 and mix["colours"] == [0, 1] and mix["crossed_and_lost"] >= 1 and mix["false_positives"] >= 1 and mix["old_way"] >= 1
    want = dict(capture=dict(games=12, resigned=3, by=[1, 2], playon=4, lost=1, fp=1, old=7),
                xiangqi=dict(games=11, resigned=5, by=[2, 3], playon=3, lost=1, fp=2, old=3))[level]
    oc = [o for _, _, o in out["outcomes"]]
    by = [sum(1 for o in oc if o.how == "resign" and o.result == w) for w in ("black", "red")]           # red resigned: black wins
    assert (len(oc), mix["resigned"], by, mix["crossed_and_lost"], mix["false_positives"], mix["old_way"]) == \
        (want["games"], want["resigned"], want["by"], want["lost"], want["fp"], want["old"])
    rs = out["resign_stats"]
    assert rs == dict(resigned=want["resigned"], playon_games=want["playon"], playon_would_resign=want["lost"] + want["fp"],
                      playon_false_positives=want["fp"])
    assert out["min_margin"] >= 1e-9 and out["stats"]["stalled"] == 0 and int(out["game_no"].max()) >= 2
    # the records of a resigned game: every ply it played, z from the resigner's loss
    from cchess_zero_amd.selfplay import unpack_records
    at = 0
    for t, g, o in out["outcomes"]:
        rec = unpack_records(out["records"][at:at + o.fin_n])
        at += o.fin_n
        assert rec["ply"].tolist() == list(range(o.fin_n))
        if o.how == "resign":
            winner = 0 if o.result == "red" else 1
            assert not o.playon and (rec["z"] == np.where(rec["side"] == winner, 1, -1)).all()
    assert at == len(out["records"])
    # the histogram holds one entry per judged side that did not lose a play-on game, the lowest value a false positive had is below the threshold
    assert 0 < out["hist"].sum() <= 2 * rs["playon_games"] and out["hist"][:R.hist_bin(np.float32(-0.125))].sum() >= rs["playon_false_positives"]


def test_play_on_everywhere_plays_the_games_without_resignation():
    for level in sorted(R.LEVELS):
        on, off = R.sp_model(level, playon=1.0), R.sp_model(level, off=True)
        assert on["records"].tobytes() == off["records"].tobytes() and on["stats"] == off["stats"]
        assert on["resign_stats"]["resigned"] == 0 and on["resign_stats"]["playon_games"] == on["stats"]["games"] > 0
        assert off["resign_stats"] == dict.fromkeys(R.STATS, 0) and not off["hist"].any()


def test_the_histogram_bins():
    f = np.float32
    assert [R.hist_bin(f(q)) for q in (-1.0, -0.96875, -0.125, -0.0625, 0.0, 0.999, 1.0, -1.5, 3.0)] == [0, 1, 28, 30, 32, 63, 63, 0, 63]
    assert R.hist_bin(f(-0.1251)) == 27 and R.hist_bin(np.nextafter(f(-0.125), f(1))) == 28
    # q + 1.0f is rounded to float32 before the floor, as in the kernel: the value next below an edge can land in the edge's bin
    assert R.hist_bin(np.nextafter(f(-0.125), f(-1))) == 28 and R.hist_bin(np.nextafter(f(-0.75), f(-1))) == 7
