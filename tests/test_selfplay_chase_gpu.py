"""Self-play with the perpetual-chase rule on the GPU (cz_selfplay_set_chase, csrc/cz_selfplay.hip) against
tests/selfplay_rules_model.py: whole games byte for byte, the constructed chase (ply 8, a loss for red, counted as a chase and
not as a perpetual check), chase off as self-play was, and the setter's refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import chase_cases as CC
import chase_model as CM
import fakenet
import match_model as MM
import repetition_cases as RC
from test_selfplay_chase_cpu import WHOLE, whole_games_model, whole_games_stream

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
EINVAL = -1
STATS = ("games", "red_wins", "black_wins", "draws", "plies", "stalled", "mates", "repetitions", "perpetuals")


def _selfplay(boards, side, playouts, cap=1 << 14, **kw):
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    boards = np.asarray(boards, np.uint8).reshape(-1, 90)
    eng = SearchEngine(len(boards), cap, plane_dtype=torch.float32, channels=14)
    sp = SelfPlay(eng, None, playouts, **kw)
    sp.start(boards, np.asarray(side, np.uint8), np.zeros(len(boards), np.int32))
    return eng, sp


def _run_whole_games(**extra):
    boards, side = RC.cpu_openings(WHOLE["G"], 4, 11)
    eng, sp = _selfplay(boards, side, WHOLE["playouts"], cap=1 << 15, exploration=False, temperature=WHOLE["temperature"], continuous=False,
                        max_plies=WHOLE["max_plies"], rules="xiangqi", repetition=3, **extra)
    fwd = MM.device_forward("pos", 11)
    for rand in whole_games_stream():
        sp.step_ply(fwd, rand=rand)
    return sp.drain(), sp.stats(), sp.active().numpy().astype(bool)


def test_whole_games_equal_the_model():
    want = whole_games_model()
    print("model:", want["stats"], "min margin %.3g over %d picks" % (want["min_margin"], want["picks"]))
    assert want["min_margin"] >= 1e-12 and want["picks"] == want["stats"]["plies"] and not want["active"].any()
    assert want["stats"]["chases"] >= 1 and want["stats"]["repetitions"] >= 1
    rec, st, active = _run_whole_games(chase=True)
    assert {k: st[k] for k in STATS + ("chases",)} == want["stats"] and st["dropped"] == 0
    assert np.array_equal(active, want["active"])
    assert rec.shape == want["records"].shape and np.array_equal(rec, want["records"])


def test_chase_off_is_selfplay_as_it_was():
    want = whole_games_model(chase=False)
    rows = [_run_whole_games(), _run_whole_games(chase=False)]
    assert rows[0][0].tobytes() == rows[1][0].tobytes() and rows[0][1] == rows[1][1] and "chases" not in rows[0][1]
    assert np.array_equal(rows[0][0], want["records"]) and {k: rows[0][1][k] for k in STATS} == {k: want["stats"][k] for k in STATS}


def test_the_constructed_chase_ends_at_ply_8_as_a_loss_for_red():
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.selfplay import unpack_records
    l2i = tables()["label2i"]
    line = [int(l2i[m]) for m in CC.CHASE_LINE]
    boards, sides, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE)
    want = CM.records(boards, sides)
    fwd = MM.device_forward("pos", 11)
    u = (None, np.full(1, 0.5, np.float32))
    eng, sp = _selfplay([CC.CHASE_BOARD], [0], 8, exploration=False, continuous=True, rules="xiangqi", repetition=3, chase=True)
    for game in (1, 2):                 # the second game of the slot: re-seeded in place, the rings are not cleared
        for t in range(8):
            sp.step_ply(fwd, forced=np.array([line[t]], np.uint16), rand=u)
            assert sp.fin_n.cpu().tolist() == [0], (game, t)
        sp.step_ply(fwd, forced=np.array([line[0]], np.uint16), rand=u)
        assert sp.played.cpu().numpy().view(np.uint16).tolist() == [NONE] and sp.fin_n.cpu().tolist() == [8]
        ring = sp.chase_history()
        assert np.array_equal(ring[0, :9], want)
        rec = unpack_records(sp.drain())
        assert rec["ply"].tolist() == list(range(8)) and rec["z"].tolist() == [-1, 1] * 4       # red chased: black wins
        st = sp.stats()
        assert (st["games"], st["black_wins"], st["red_wins"], st["draws"]) == (game, game, 0, 0)
        assert (st["chases"], st["perpetuals"], st["repetitions"], st["mates"]) == (game, 0, 0, 0)
    # without the chase rule the same line is a draw by repetition
    eng, sp = _selfplay([CC.CHASE_BOARD], [0], 8, exploration=False, continuous=True, rules="xiangqi", repetition=3)
    for t in range(9):
        sp.step_ply(fwd, forced=np.array([line[t % 4]], np.uint16), rand=u)
    st = sp.stats()
    assert (st["games"], st["draws"], st["repetitions"], st["perpetuals"]) == (1, 1, 1, 0) and "chases" not in st
    from cchess_zero_amd._lib import CchessHipError
    with pytest.raises(CchessHipError, match="cz_selfplay_set_chase first"):
        sp.chase_history()


def test_set_chase_refuses_what_it_cannot_keep():
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import SearchEngine
    L = lib()
    err = lambda: (L.cz_last_error() or b"").decode()
    eng = SearchEngine(2, 1 << 12, plane_dtype=torch.float32, channels=14)
    eng.reset(np.stack([CC.CHASE_BOARD] * 2), np.zeros(2, np.uint8), None)
    h = eng.ctx.h
    begin = lambda: check(L.cz_selfplay_begin(h, 16, None, None, None), "cz_selfplay_begin")
    assert L.cz_selfplay_set_chase(h, 1) == EINVAL and "cz_selfplay_begin first" in err()
    begin()
    assert L.cz_selfplay_set_chase(h, 1) == EINVAL and "cz_selfplay_set_repetition(ctx, fold) first" in err()      # needs a fold
    assert L.cz_selfplay_chase_history(h, None) == EINVAL
    assert L.cz_selfplay_set_rules(h, 1) == 0 and L.cz_selfplay_set_repetition(h, 3) == 0
    for on in (2, -1):
        assert L.cz_selfplay_set_chase(h, on) == EINVAL
    assert L.cz_selfplay_set_chase(h, 1) == 0
    assert L.cz_selfplay_set_repetition(h, 0) == EINVAL and "cz_selfplay_set_chase(ctx, 0) first" in err()
    p = C.c_void_p()
    assert L.cz_selfplay_chase_history(h, C.byref(p)) == 0 and p.value
    stat = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    eng.ctx.bind_stream()
    assert L.cz_selfplay_chase_stats(h, C.c_void_p(stat.data_ptr())) == 0 and int(stat.item()) == 0
    assert L.cz_selfplay_chase_stats(h, None) == EINVAL
    begin()                                                                               # cz_selfplay_begin switches it off
    assert L.cz_selfplay_chase_history(h, None) == EINVAL
    assert L.cz_selfplay_set_rules(h, 1) == 0 and L.cz_selfplay_set_repetition(h, 3) == 0 and L.cz_selfplay_set_chase(h, 1) == 0
    eng.search(MM.device_forward("pos", 11), 4)
    u = torch.full((2,), 0.5, dtype=torch.float32, device="cuda")
    played = torch.empty(2, dtype=torch.int16, device="cuda")
    eng.ctx.bind_stream()
    check(L.cz_selfplay_choose(h, None, C.c_void_p(u.data_ptr()), None, 1.0, 0.0, 0, C.c_void_p(played.data_ptr())), "cz_selfplay_choose")
    torch.cuda.synchronize()
    assert L.cz_selfplay_set_chase(h, 0) == EINVAL and "before the first cz_selfplay_choose" in err()
    begin()
    torch.cuda.synchronize()
