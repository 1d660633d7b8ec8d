"""Self-play with resignation on the GPU (cz_selfplay_set_resign, csrc/cz_selfplay.hip) against tests/resign_model.py: the fixture
of tests/resign_model.SP — parked and re-seeded slots, king-capture rules and xiangqi + fold 3 + chase — record for record with the
counters and the histogram; every game playing on against resignation off; asynchronous plies; forced labels; retuning."""
import numpy as np
import pytest
import torch

import match_model as MM
import resign_model as R

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
STATS = ("games", "red_wins", "black_wins", "draws", "plies", "stalled")
XQ_STATS = ("mates", "repetitions", "perpetuals", "chases")


def _selfplay(boards, side, playouts, cap=1 << 15, **kw):
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    boards = np.asarray(boards, np.uint8).reshape(-1, 90)
    eng = SearchEngine(len(boards), cap, plane_dtype=torch.float32, channels=14)
    sp = SelfPlay(eng, None, playouts, **kw)
    sp.start(boards, np.asarray(side, np.uint8), np.zeros(len(boards), np.int32))
    return eng, sp


def _run(level, continuous=True, retune=None, off=False, **over):
    """The fixture on the device -> (records in ring order, stats, histogram, active)."""
    lv, rs = R.LEVELS[level], R.SP["resign"]
    kw = {} if off else dict(dict(resign=rs["threshold"], resign_min_ply=rs["min_ply"], resign_playon=rs["playon"]), **over)
    boards, side = R.sp_openings()
    eng, sp = _selfplay(boards, side, R.SP["playouts"], exploration=True, temperature=R.SP["temperature"], continuous=continuous,
                        max_plies=R.SP["max_plies"], seed=rs["seed"], rules=lv["rules"], repetition=lv["fold"], chase=lv["chase"], **kw)
    fwd = MM.device_forward("pos", 11)
    for t, rand in enumerate(R.sp_stream()):
        if retune and t in retune:
            sp.set_resign_threshold(retune[t])
        sp.step_ply(fwd, rand=rand)
    return sp.drain(), sp.stats(), sp.resign_histogram(), sp.active().numpy().astype(bool)


def _assert_equals_model(got, want, level, tag):
    rec, st, hist, active = got
    keys = STATS + (XQ_STATS if level == "xiangqi" else ())
    assert {k: st[k] for k in keys} == {k: want["stats"][k] for k in keys}, (tag, st, want["stats"])
    assert {k: st[k] for k in R.STATS} == want["resign_stats"], (tag, st, want["resign_stats"])
    assert np.array_equal(hist, want["hist"]), (tag, hist, want["hist"])
    assert np.array_equal(active, want["active"]) and st["dropped"] == 0
    assert rec.shape == want["records"].shape and np.array_equal(rec, want["records"]), tag


# ---- 1. the fixture, record for record ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("level", sorted(R.LEVELS))
def test_resigning_selfplay_equals_the_model(level, continuous):
    want = R.sp_model(level, continuous=continuous)
    mix = R.sp_mix(R.sp_model(level))
    print("model:", level, continuous, want["stats"], want["resign_stats"], "margin %.3g" % want["min_margin"], "game_no", want["game_no"].tolist())
    assert mix["resigned"] >= 2 and mix["colours"] == [0, 1] and mix["crossed_and_lost"] >= 1 and mix["false_positives"] >= 1 and mix["old_way"] >= 1
    assert want["min_margin"] >= 1e-9 and want["resign_stats"]["resigned"] >= 1 and want["resign_stats"]["playon_games"] >= 1
    assert int(want["game_no"].max()) >= (2 if continuous else 0) and want["active"].all() == continuous
    _assert_equals_model(_run(level, continuous), want, level, (level, continuous))


# ---- 2. every game plays on: self-play as it was, counted ------------------------------------------------------------------------------
def test_play_on_everywhere_is_selfplay_without_resignation():
    on, off = _run("capture", resign_playon=1.0), _run("capture", off=True)
    assert on[0].tobytes() == off[0].tobytes() and len(on[0]) > 0
    for k in STATS + ("dropped", "sims"):
        assert on[1][k] == off[1][k], k
    assert on[1]["resigned"] == 0 and on[1]["playon_games"] == on[1]["games"] > 0 and on[1]["playon_would_resign"] >= 1 and on[2].sum() > 0
    assert not any(k in off[1] for k in R.STATS) and not off[2].any()
    _assert_equals_model(on, R.sp_model("capture", playon=1.0), "capture", "playon 1")


# ---- 3. asynchronous plies ----------------------------------------------------------------------------------------------------------
def test_asynchronous_plies_end_a_resigned_game_that_did_not_move():
    """Threshold +2: every judged ply resigns.  min_ply 4, nobody plays on, from the start position: every game is 4 plies long
    and red, to move at ply 4, resigns it — the slot's played is 0xFFFF then, which the asynchronous adjudication otherwise skips."""
    from cchess_zero_amd.rules import START_BOARD
    from cchess_zero_amd.selfplay import unpack_records
    G = 8
    eng, sp = _selfplay(np.tile(START_BOARD, (G, 1)), np.zeros(G, np.uint8), 4, cap=1 << 12, exploration=True, continuous=True, max_plies=64,
                        seed=3, resign=2.0, resign_min_ply=4, resign_playon=0.0)
    sp.run_async(96, MM.device_forward("pos", 11), every=2)
    st = sp.stats()
    rec = unpack_records(sp.drain())
    assert st["games"] >= G and st["resigned"] == st["games"] == st["black_wins"] and st["plies"] == 4 * st["games"] == len(rec["ply"])
    assert (st["stalled"], st["draws"], st["red_wins"], st["playon_games"], st["dropped"]) == (0, 0, 0, 0, 0)
    assert rec["ply"].reshape(-1, 4).tolist() == [[0, 1, 2, 3]] * st["games"] and rec["side"].reshape(-1, 4).tolist() == [[0, 1, 0, 1]] * st["games"]
    assert rec["z"].reshape(-1, 4).tolist() == [[-1, 1, -1, 1]] * st["games"]
    assert not sp.resign_histogram().any()


# ---- 4. a forced label is played, not judged -------------------------------------------------------------------------------------------
def test_a_forced_label_suppresses_the_judgement():
    from cchess_zero_amd.rules import START_BOARD
    from cchess_zero_amd.selfplay import unpack_records
    eng, sp = _selfplay(np.tile(START_BOARD, (2, 1)), np.zeros(2, np.uint8), 8, cap=1 << 12, exploration=False, continuous=True, max_plies=64,
                        resign=2.0, resign_playon=0.0)
    fwd = MM.device_forward("pos", 11)
    u = (None, np.full(2, 0.5, np.float32))

    def ply(force):
        """One lock-step ply: slots with force[g] play their root's first child as a forced label, the others choose."""
        eng.search(fwd, sp.playouts)
        first = eng.root_stats_host()["label"][:, 0]
        forced = np.where(force, first, NONE).astype(np.uint16)
        sp._transition(0, forced, u)
        return sp.played.cpu().numpy().view(np.uint16).tolist(), sp.fin_n.cpu().tolist(), [int(x) for x in forced]

    played, fin, forced = ply([True, False])          # slot 1 is judged at ply 0 and resigns a game of no ply
    assert played == [forced[0], NONE] and fin == [0, 0]
    st = sp.stats()
    assert (st["games"], st["resigned"], st["black_wins"], st["plies"]) == (1, 1, 1, 0)
    played, fin, forced = ply([True, True])
    assert played == forced and fin == [0, 0] and sp.stats()["games"] == 1
    played, fin, forced = ply([False, True])          # slot 0, two forced plies played, is judged now: red resigns
    assert played == [NONE, forced[1]] and fin == [2, 0]
    st = sp.stats()
    assert (st["games"], st["resigned"], st["black_wins"], st["plies"], st["stalled"]) == (2, 2, 2, 2, 0)
    rec = unpack_records(sp.drain())
    assert rec["ply"].tolist() == [0, 1] and rec["side"].tolist() == [0, 1] and rec["z"].tolist() == [-1, 1]


# ---- 5. retuning ---------------------------------------------------------------------------------------------------------------------
def test_retuning_keeps_the_games_their_numbers_and_the_counters():
    want = R.sp_model("capture", retune_at=20, retune_to=-0.0625)
    same = R.sp_model("capture")
    at = [t for t, _, o in want["outcomes"] if o.how == "resign"]
    print("model:", want["stats"], want["resign_stats"], "resigned at", at, "game_no", want["game_no"].tolist())
    assert min(at) < 20 <= max(at) and want["records"].tobytes() != same["records"].tobytes() and int(want["game_no"].max()) >= 2
    assert any(o.playon and o.game_no >= 1 for _, _, o in want["outcomes"])       # a play-on draw that needs the slot's game number
    _assert_equals_model(_run("capture", retune={20: -0.0625}), want, "capture", "retune")
