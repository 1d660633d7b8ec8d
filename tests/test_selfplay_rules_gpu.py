"""Self-play under rules="xiangqi" on the GPU (cz_selfplay_set_rules / cz_selfplay_set_repetition, csrc/cz_selfplay.hip)
against tests/selfplay_rules_model.py: a mate ends the game, pi and the move are over the king-safe root children, whole games
equal the model byte for byte, repetition and perpetual check, the setters' refusals, rules="capture" as self-play was, and the
asynchronous loop feeding a policy update."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import fakenet
import kingsafe_model as KM
import match_model as MM
import repetition_cases as RC
import selfplay_rules_model as XS
from test_match_gpu import _const_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFF
EINVAL = -1
QUIET_LINE = ["e5e4", "d9d8", "e4e5", "d8d9"]
STATS = ("games", "red_wins", "black_wins", "draws", "plies", "stalled")
XQ_STATS = ("mates", "repetitions", "perpetuals")


def _board(fen):
    from oracle import oracle as O
    return O.fen_to_board(fen)


def _labels(names):
    from cchess_zero_amd._lib import tables
    l2i = tables()["label2i"]
    return [int(l2i[n]) for n in names]


def _selfplay(boards, side, playouts, cap=1 << 14, **kw):
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    boards = np.asarray(boards, np.uint8).reshape(-1, 90)
    eng = SearchEngine(len(boards), cap, plane_dtype=torch.float32, channels=14)
    sp = SelfPlay(eng, None, playouts, **kw)
    sp.start(boards, np.asarray(side, np.uint8), np.zeros(len(boards), np.int32))
    return eng, sp


def _u(G, value=0.5):
    return (None, np.full(G, value, np.float32))


def _forced(labels):
    return np.asarray(labels, np.uint16)


# ---- 1. mate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fen,side,move", [("4K4/8r/9/9/9/r8/9/9/9/3k5", 1, "a5a0"), ("3K5/9/9/9/R8/9/9/9/8R/4k4", 0, "a4a9")])
def test_mate_ends_the_game(fen, side, move):
    from cchess_zero_amd.selfplay import unpack_records
    b, mv = _board(fen), _labels([move])[0]
    fwd = MM.device_forward("pos", 11)
    eng, sp = _selfplay([b], [side], 8, exploration=False, continuous=False, rules="xiangqi")
    sp.step_ply(fwd, forced=_forced([mv]), rand=_u(1))
    assert sp.fin_n.cpu().tolist() == [0] and bool(sp.active().all())
    sp.step_ply(fwd, rand=_u(1))
    assert sp.played.cpu().numpy().view(np.uint16).tolist() == [NONE]
    assert sp.fin_n.cpu().tolist() == [1] and not bool(sp.active().any())
    u = unpack_records(sp.drain())
    safe = KM.kingsafe(b, side)[0]
    assert u["side"].tolist() == [side] and u["z"].tolist() == [1] and u["ply"].tolist() == [0]
    assert np.array_equal(u["boards"][0], b) and u["counts"].tolist() == [len(safe)] and np.array_equal(u["labels"][0, :len(safe)], safe)
    st = sp.stats()
    assert (st["games"], st["plies"], st["mates"], st["repetitions"], st["perpetuals"], st["draws"], st["stalled"]) == (1, 1, 1, 0, 0, 0, 0)
    assert (st["red_wins"], st["black_wins"]) == ((0, 1) if side else (1, 0))
    root = eng.root_state()[0].cpu().numpy()[0]
    assert (root == 1).any() and (root == 8).any()            # no king was taken
    # under king-capture rules the same two plies do not end the game: the mated side moves, and loses its king a ply later
    eng, sp = _selfplay([b], [side], 8, exploration=False, continuous=False, rules="capture")
    sp.step_ply(fwd, forced=_forced([mv]), rand=_u(1))
    sp.step_ply(fwd, rand=_u(1))
    assert sp.fin_n.cpu().tolist() == [0] and bool(sp.active().all()) and sp.stats()["games"] == 0
    assert "mates" not in sp.stats()


# ---- 2. the most visited child is unsafe ------------------------------------------------------------------------------------
def test_the_record_and_the_move_leave_out_an_unsafe_most_visited_child():
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.selfplay import to_dense, unpack_records
    from oracle import oracle as O
    b = _board("4K4/9/9/4R4/9/9/9/9/4r4/3k5")
    unsafe = int(tables()["lut"][4, 3])
    safe = KM.kingsafe(b, 0)[0]
    pseudo = O.legal_moves(b, 0)
    assert len(pseudo) == 18 and len(safe) == 9 and unsafe not in set(safe.tolist())
    fwd = _const_forward(0.5, prefer=[unsafe])
    for rules, want in (("xiangqi", safe), ("capture", pseudo)):
        eng, sp = _selfplay([b], [0], 40, exploration=False, continuous=False, max_plies=1, rules=rules)   # one ply: the record is flushed
        eng.search(fwd, 40)
        st = eng.root_stats_host()
        n = int(st["count"][0])
        vis, lab = st["N"][0, :n], st["label"][0, :n]
        top = int(np.argmax(vis))
        assert n == 18 and int(lab[top]) == unsafe and (vis[top] > np.delete(vis, top)).all()     # not vacuous: the unsafe child leads
        sp.playouts = 0                                    # the search is done: choose / advance / adjudicate / flush
        sp.step_ply(fwd, rand=_u(1, 0.0))                  # u = 0: the first child with a positive probability
        played = int(sp.played.cpu().numpy().view(np.uint16)[0])
        rec = sp.drain()
        u = unpack_records(rec)
        keep = [i for i, l in enumerate(lab) if int(l) in set(want.tolist())]
        assert u["counts"].tolist() == [len(want)] and np.array_equal(u["labels"][0, :len(want)], want)
        assert np.array_equal(u["visits"][0, :len(want)], vis[keep]) and (u["labels"][0, len(want):] == NONE).all() and not u["visits"][0, len(want):].any()
        assert played == int(lab[[i for i in keep if vis[i] > 0][0]])
        if rules == "xiangqi":
            assert played in set(safe.tolist()) and played != unsafe
            assert to_dense(rec)[1][0, unsafe] == 0.0      # pi has no mass on the unsafe move
        else:
            assert played == unsafe


# ---- 3. whole games --------------------------------------------------------------------------------------------------------
def test_whole_games_equal_the_model():
    """16 openings, 16 playouts, 41 lock-step plies at temperature 0.05 with max_plies 40.  The stream (seed 1, chosen on the CPU
    with the model): slots 0-7 get Dirichlet noise, slots 8-15 gamma rows of zeros (the kernel's no-noise case), so some of them
    shuffle into a threefold repetition."""
    G, T, playouts, max_plies, temperature = 16, 41, 16, 40, 0.05
    boards, side = RC.cpu_openings(G, 4, 11)
    rng = np.random.default_rng(1)
    stream = [(rng.gamma(0.3, size=(G, 128)).astype(np.float32), rng.random(G).astype(np.float32)) for _ in range(T)]
    for gamma, _ in stream:
        gamma[8:] = 0
    want = XS.play_games(fakenet.make_forward("pos", 11), playouts, boards, side, None, stream, max_plies=max_plies,
                         temperature=temperature, fold=3)
    print("model:", want["stats"], "min margin %.3g over %d picks, %d plies with an unsafe child" % (want["min_margin"], want["picks"], want["unsafe_plies"]))
    # the comparison is exact and not vacuous: no pick sits on a CDF boundary, none is left out, the filter and the rule act
    assert want["min_margin"] >= 1e-12 and want["picks"] == want["stats"]["plies"]
    assert want["unsafe_plies"] >= 1 and want["stats"]["repetitions"] >= 1 and not want["active"].any()
    eng, sp = _selfplay(boards, side, playouts, cap=1 << 15, exploration=True, temperature=temperature, continuous=False,
                        max_plies=max_plies, rules="xiangqi", repetition=3)
    fwd = MM.device_forward("pos", 11)
    for t in range(T):
        sp.step_ply(fwd, rand=stream[t])
    rec = sp.drain()
    st = sp.stats()
    assert {k: st[k] for k in STATS + XQ_STATS} == {k: want["stats"][k] for k in STATS + XQ_STATS} and st["dropped"] == 0
    assert np.array_equal(sp.active().numpy().astype(bool), want["active"])
    assert rec.shape == want["records"].shape and np.array_equal(rec, want["records"])


# ---- 4. repetition -----------------------------------------------------------------------------------------------------------
def test_repetition_and_perpetual_check_end_the_game_at_ply_8():
    from cchess_zero_amd.selfplay import unpack_records
    b = RC.perpetual_board()
    lines = [_labels(RC.PERPETUAL_LINE), _labels(QUIET_LINE)]
    hist = [XS.replay_line(b, 0, line * 2, fold=3) for line in lines]
    assert [(h["ply"], h["code"]) for h in hist] == [(8, XS.RM.RED_LOSES), (8, XS.RM.DRAW)]
    fwd = MM.device_forward("pos", 11)
    forced = lambda t: _forced([lines[0][t % 4], lines[1][t % 4]])
    eng, sp = _selfplay([b, b], [0, 0], 8, exploration=False, continuous=True, rules="xiangqi", repetition=3)
    for game in (1, 2):                 # the second game of each slot: re-seeded in place, the ring is not cleared
        for t in range(8):
            sp.step_ply(fwd, forced=forced(t), rand=_u(2))
            assert sp.fin_n.cpu().tolist() == [0, 0], (game, t)
        sp.step_ply(fwd, forced=forced(8), rand=_u(2))
        assert sp.played.cpu().numpy().view(np.uint16).tolist() == [NONE, NONE]
        assert sp.fin_n.cpu().tolist() == [8, 8], game
        keys, checks = sp.history()
        for g in (0, 1):
            for i in range(9):
                assert int(keys[g, i & 63]) == hist[g]["keys"][i] and int(checks[g, i & 63]) == hist[g]["checks"][i], (game, g, i)
        u = unpack_records(sp.drain())
        assert u["ply"].tolist() == list(range(8)) * 2 and u["side"].tolist() == [0, 1] * 8
        assert u["z"][:8].tolist() == [-1, 1] * 4           # red checked perpetually: black wins
        assert not u["z"][8:].any()                         # the quiet shuffle: a draw
        st = sp.stats()
        assert (st["games"], st["black_wins"], st["red_wins"], st["draws"], st["plies"]) == (2 * game, game, 0, game, 16 * game)
        assert (st["mates"], st["repetitions"], st["perpetuals"]) == (0, game, game)
        assert bool(sp.active().all())
    # without the rule neither game ends at ply 8
    eng, sp = _selfplay([b, b], [0, 0], 8, exploration=False, continuous=True, rules="xiangqi", repetition=0)
    for t in range(9):
        sp.step_ply(fwd, forced=forced(t), rand=_u(2))
    st = sp.stats()
    assert st["games"] == 0 and (st["mates"], st["repetitions"], st["perpetuals"]) == (0, 0, 0)
    assert sp.played.cpu().numpy().view(np.uint16).tolist() == [lines[0][0], lines[1][0]]
    from cchess_zero_amd._lib import CchessHipError
    with pytest.raises(CchessHipError, match="cz_selfplay_set_repetition first"):
        sp.history()


# ---- 5. the setters ----------------------------------------------------------------------------------------------------------
def test_the_setters_refuse_what_they_cannot_keep():
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import SearchEngine
    L = lib()
    err = lambda: (L.cz_last_error() or b"").decode()
    eng = SearchEngine(2, 1 << 12, plane_dtype=torch.float32, channels=14)
    b = RC.perpetual_board()
    eng.reset(np.stack([b, b]), np.zeros(2, np.uint8), None)
    h = eng.ctx.h
    begin = lambda: check(L.cz_selfplay_begin(h, 16, None, None, None), "cz_selfplay_begin")
    # before cz_selfplay_begin
    assert L.cz_selfplay_set_rules(h, 1) == EINVAL and "cz_selfplay_begin first" in err()
    assert L.cz_selfplay_set_repetition(h, 0) == EINVAL and "cz_selfplay_begin first" in err()
    begin()
    assert L.cz_selfplay_set_repetition(h, 3) == EINVAL and "cz_selfplay_set_rules(ctx, 1) first" in err()     # needs rules 1
    assert L.cz_selfplay_history(h, None, None) == EINVAL
    for rules in (2, -1):
        assert L.cz_selfplay_set_rules(h, rules) == EINVAL
    assert L.cz_selfplay_set_rules(h, 1) == 0
    for fold in (1, 9, -1):
        assert L.cz_selfplay_set_repetition(h, fold) == EINVAL and "2..8" in err()
    assert L.cz_selfplay_set_repetition(h, 3) == 0 and L.cz_selfplay_set_repetition(h, 0) == 0 and L.cz_selfplay_set_repetition(h, 8) == 0
    assert L.cz_selfplay_set_rules(h, 0) == EINVAL and "cz_selfplay_set_repetition(ctx, 0) first" in err()     # not while the fold is set
    pk, pc = C.c_void_p(), C.c_void_p()
    assert L.cz_selfplay_history(h, C.byref(pk), C.byref(pc)) == 0 and pk.value and pc.value
    # cz_selfplay_begin resets both settings
    begin()
    assert L.cz_selfplay_history(h, None, None) == EINVAL                                # fold 0 again
    assert L.cz_selfplay_set_repetition(h, 3) == EINVAL                                  # rules 0 again
    assert L.cz_selfplay_set_rules(h, 1) == 0 and L.cz_selfplay_set_repetition(h, 3) == 0
    # after a cz_selfplay_choose
    eng.search(MM.device_forward("pos", 11), 4)
    u = torch.full((2,), 0.5, dtype=torch.float32, device="cuda")
    played = torch.empty(2, dtype=torch.int16, device="cuda")
    eng.ctx.bind_stream()
    check(L.cz_selfplay_choose(h, None, C.c_void_p(u.data_ptr()), None, 1.0, 0.0, 0, C.c_void_p(played.data_ptr())), "cz_selfplay_choose")
    torch.cuda.synchronize()
    for call in (lambda: L.cz_selfplay_set_rules(h, 1), lambda: L.cz_selfplay_set_repetition(h, 0),
                 lambda: L.cz_selfplay_set_repetition(h, 2), lambda: L.cz_selfplay_set_rules(h, 0)):
        assert call() == EINVAL and "before the first cz_selfplay_choose" in err()
    begin()
    assert L.cz_selfplay_set_rules(h, 1) == 0
    torch.cuda.synchronize()


# ---- 6. capture by name ------------------------------------------------------------------------------------------------------
def test_capture_rules_by_name_are_selfplay_as_it_was():
    from oracle import oracle as O
    G = 8
    boards, side = np.tile(O.fen_to_board(O.START_FEN), (G, 1)), np.zeros(G, np.uint8)
    fwd = MM.device_forward("pos", 11)
    rows = []
    for extra in ({}, dict(rules="capture", repetition=0)):
        eng, sp = _selfplay(boards, side, 12, exploration=True, seed=7, continuous=True, max_plies=5, **extra)
        for _ in range(12):
            sp.step_ply(fwd)
        rows.append((sp.drain(), sp.stats()))
    assert len(rows[0][0]) == 2 * 5 * G and np.array_equal(rows[0][0], rows[1][0])
    assert rows[0][1] == rows[1][1] and "mates" not in rows[1][1]


# ---- 7. the asynchronous loop ------------------------------------------------------------------------------------------------
def test_asynchronous_xiangqi_selfplay_feeds_a_policy_update(tmp_path):
    from cchess_zero_amd.selfplay import to_dense, unpack_records
    from cchess_zero_amd.train import policy_update
    from oracle import oracle as O
    G, playouts = 16, 16
    boards, side = np.tile(O.fen_to_board(O.START_FEN), (G, 1)), np.zeros(G, np.uint8)
    eng, sp = _selfplay(boards, side, playouts, exploration=True, seed=3, continuous=True, max_plies=10, rules="xiangqi", repetition=3)
    sp.run_async(240, MM.device_forward("pos", 11), every=8)
    rec = sp.drain()
    st = sp.stats()
    print("asynchronous xiangqi self-play:", st)
    assert st["games"] >= G and st["stalled"] == 0 and st["dropped"] == 0 and len(rec) == st["plies"]
    assert st["red_wins"] + st["black_wins"] == st["mates"] + st["perpetuals"]      # a legal start position: no king is ever taken
    assert st["games"] == st["red_wins"] + st["black_wins"] + st["draws"] and st["repetitions"] <= st["draws"]
    u = unpack_records(rec)
    for i in range(len(rec)):
        safe = KM.kingsafe(u["boards"][i], int(u["side"][i]))[0]           # every pseudo-legal move is a root child
        k = int(u["counts"][i])
        assert k == len(safe) and np.array_equal(u["labels"][i, :k], safe), i
        assert (u["labels"][i, k:] == NONE).all() and not u["visits"][i, k:].any()
    planes, pi, z = to_dense(rec)
    assert np.allclose(pi.sum(axis=1), 1.0, atol=1e-12)
    sys.path.insert(0, ROOT)
    from policy_value_network import policy_value_network
    net = policy_value_network(2, save_dir=str(tmp_path), seed=3)
    n = min(32, len(rec))
    _, info = policy_update(net, list(rec[:n]), n, 1, 0.02, 1.0, 0.025, log=lambda *a: None, sample=range(n), save=False)   # packed records, as main.py's buffer
    assert info["steps"] == 1 and np.isfinite(float(info["loss"]))
