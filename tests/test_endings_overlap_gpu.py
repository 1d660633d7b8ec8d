"""Two endings at once, on the GPU: the match (csrc/cz_match.hip) and self-play (csrc/cz_selfplay.hip) driven into hand-set
positions in which two endings of wave_game_end's precedence (csrc/cz_internal.h) hold together, against tests/match_model.py /
tests/resign_model.py.  A uniform forward (logits 0, value 0) at 8 playouts: every tried child has one visit, the greedy move is
the first generated one.

  NOBODY     red to move and no red piece on the board: no child to play on a board whose king is gone — aborted / stalled, not a
             king capture
  TAKES      black's first move takes the red king, max_plies 1: a king capture, not the ply cap
  QUIET      restrict_round 59 and a quiet move, max_plies 1: 60 plies without a capture, not the ply cap
  MATED      xiangqi, resignation at +2 (every judged value is below it): the mover is mated — mate, not resignation
  MATES      xiangqi, fold 2: black's first move mates; the ring then gets the mate position's key as position 0, so the mated root is
             a second occurrence, reached by a checking move of black alone — perpetual check (black loses), not mate (red loses)
"""
import ctypes as C

import numpy as np
import pytest

import chase_cases as CC
import match_model as MM
import resign_model as R

NONE = 0xFFFF
PLAYOUTS = 8
NOBODY = CC.board([], kings=("ke9",))
TAKES = CC.board(["re1"], kings=("Kd1", "ke9"))
QUIET = CC.board(["Ra4"])
MATED = CC.board(["Ra9", "Rh8"], kings=("Kd0", "ke9"))                       # black to move
MATES = CC.board(["pe2", "ng2", "rd8"], kings=("Ke0", "ke9"))                # black to move: e2e1 mates
MATE_POSITION = CC.board(["pe1", "ng2", "rd8"], kings=("Ke0", "ke9"))        # red to move


def uniform_forward(planes):
    n = 1 if np.ndim(planes) == 3 else len(planes)
    return np.zeros((n, 2086), np.float32), np.zeros((n, 1), np.float32)


def uniform_device_forward(planes):
    import torch
    return (torch.zeros((planes.shape[0], 2086), dtype=torch.float32, device=planes.device),
            torch.zeros((planes.shape[0], 1), dtype=torch.float32, device=planes.device))


def mate_key():
    from oracle import oracle as O
    return int(O.zhash(MATE_POSITION, 0))


CPU_PLAYERS = [(uniform_forward, PLAYOUTS), (uniform_forward, PLAYOUTS)]
CAPTURE_OPENINGS = (np.stack([NOBODY, TAKES, QUIET]), np.array([0, 1, 0], np.uint8), np.array([0, 0, 59], np.int32))
RESIGN_OPENINGS = (np.stack([MATED, QUIET]), np.array([1, 0], np.uint8), np.array([0, 0], np.int32))


def model_capture_match():
    from cchess_zero_amd.arena import Openings
    return MM.play_match(CPU_PLAYERS, Openings(*CAPTURE_OPENINGS), 1)


def model_resign_match():
    from cchess_zero_amd.arena import Openings
    return R.play_match(CPU_PLAYERS, Openings(*RESIGN_OPENINGS), 8, 2.0, rules="xiangqi")


def model_verdict_match():
    return [MM.play_game(CPU_PLAYERS, MATES, 1, 0, game, 8, rules="xiangqi", fold=2, preset={0: mate_key()}) for game in (0, 1)]


def stream(G, T):
    """no noise, u = 0: the first child with a visit is played"""
    return [(None, np.zeros(G, np.float32))] * T


def model_selfplay(boards, side, rr, plies, **kw):
    return R.play_selfplay(uniform_forward, PLAYOUTS, boards, side, rr, stream(len(boards), plies), eps=0.0, **kw)


def model_capture_selfplay():
    return model_selfplay(*CAPTURE_OPENINGS, 1, max_plies=1)


def model_resign_selfplay():
    return model_selfplay(*RESIGN_OPENINGS, 3, max_plies=8, rules="xiangqi",
                          resign=dict(threshold=2.0, min_ply=0, playon=0.0, seed=1))


def model_verdict_selfplay():
    return model_selfplay(MATES[None], np.array([1], np.uint8), None, 2, max_plies=8, rules="xiangqi", fold=2,
                          preset=[{0: mate_key()}])


# ---- the device -------------------------------------------------------------------------------------------------------------------
def set_ring_key(prefix, handle, ctx, slot, ply, key):
    """ring_key[slot][ply & 63] = key, through the library's own cz_upload"""
    from cchess_zero_amd._lib import out_pointers
    ptr = out_pointers(prefix + "_history", handle, 2)[0]
    word = np.array([key], np.uint64)
    ctx.call("cz_upload", C.c_void_p(ptr.value + 8 * (64 * slot + (ply & 63))), word.ctypes.data, 8)


def device_match(openings, max_plies, plies, ring=None, **kw):
    """`plies` lock-step plies of the match on 2 slots per opening -> the per-game arrays; ring: the key uploaded as position 0
    of every slot after the first ply"""
    from cchess_zero_amd.arena import Match, Openings
    player = (uniform_device_forward, PLAYOUTS)
    m = Match(player, player, Openings(*openings), slots=2 * len(openings[0]), max_plies=max_plies, nodes_per_tree=1 << 10, **kw)
    m.start()
    try:
        for t in range(plies):
            m.step_ply()
            if ring is not None and t == 0:
                for g in range(m.G):
                    set_ring_key("cz_match", m._h, m.engines[0].ctx, g, 0, ring)
        assert m.finished()[0] == m.n_games
        return m.results()
    finally:
        m.close()


def device_selfplay(boards, side, rr, plies, ring=None, **kw):
    import torch
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    G = len(boards)
    eng = SearchEngine(G, 1 << 10, plane_dtype=torch.float32, channels=14)
    sp = SelfPlay(eng, None, PLAYOUTS, exploration=False, continuous=False, **kw)
    sp.start(np.asarray(boards, np.uint8), np.asarray(side, np.uint8), np.zeros(G, np.int32) if rr is None else rr)
    for t, rand in enumerate(stream(G, plies)):
        sp.step_ply(uniform_device_forward, rand=rand)
        if ring is not None and t == 0:
            for g in range(G):
                set_ring_key("cz_selfplay", eng.ctx.h, eng.ctx, g, 0, ring)
    return sp.drain(), sp.stats(), sp.active().numpy().astype(bool)


def assert_match(got, want):
    for k in ("result", "a_red", "plies", "reason", "moves"):
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])


def assert_selfplay(got, want, keys):
    rec, st, active = got
    ref = dict(want["stats"], **want["resign_stats"])
    assert {k: st[k] for k in keys} == {k: ref[k] for k in keys}, (st, ref)
    assert np.array_equal(active, want["active"])
    assert rec.shape == want["records"].shape and np.array_equal(rec, want["records"])


STATS = ("games", "red_wins", "black_wins", "draws", "plies", "stalled")
XQ = STATS + ("mates", "repetitions", "perpetuals")


@pytest.mark.gpu
def test_match_endings_that_hold_together():
    want = model_capture_match()
    print("capture:", want["reason"].tolist(), want["result"].tolist(), want["plies"].tolist())
    assert want["reason"].tolist() == [MM.ABORTED] * 2 + [MM.KING] * 2 + [MM.RR60] * 2 and want["plies"].tolist() == [0, 0, 1, 1, 1, 1]
    assert want["result"].tolist() == [0, 0, -1, 1, 0, 0]          # black took the king: A loses as red
    assert_match(device_match(CAPTURE_OPENINGS, 1, 1), want)

    want = model_resign_match()
    print("resign:", want["reason"].tolist(), want["result"].tolist(), want["plies"].tolist())
    assert want["reason"].tolist() == [MM.MATE] * 2 + [R.RESIGN] * 2 and want["result"].tolist()[:2] == [1, -1] and want["plies"][:2].tolist() == [0, 0]
    assert_match(device_match(RESIGN_OPENINGS, 8, int(want["plies"].max()) + 1, rules="xiangqi", resign=2.0), want)

    games = model_verdict_match()
    print("verdict:", games)
    plain = MM.play_game(CPU_PLAYERS, MATES, 1, 0, 0, 8, rules="xiangqi", fold=2)      # the ring as the game left it: red is mated
    assert (plain["reason"], plain["result"], plain["plies"], plain["moves"]) == (MM.MATE, -1, 1, games[0]["moves"])
    assert [g["reason"] for g in games] == [MM.PERPETUAL] * 2 and [g["result"] for g in games] == [1, -1] and [g["plies"] for g in games] == [1, 1]
    got = device_match((MATES[None], np.array([1], np.uint8), np.array([0], np.int32)), 8, 2, ring=mate_key(), rules="xiangqi", repetition=2)
    for g, want in enumerate(games):
        assert (got["reason"][g], got["result"][g], got["plies"][g], got["a_red"][g]) == (want["reason"], want["result"], want["plies"], want["a_red"])
        assert got["moves"][g][:2].tolist() == want["moves"] + [NONE]


@pytest.mark.gpu
def test_selfplay_endings_that_hold_together():
    want = model_capture_selfplay()
    print("capture:", want["outcomes"], want["stats"])
    assert [(g, o.result, o.fin_n) for _, g, o in want["outcomes"]] == [(0, "stalled", 0), (1, "black", 1), (2, "draw", 1)]
    assert_selfplay(device_selfplay(*CAPTURE_OPENINGS, 1, max_plies=1), want, STATS)

    want = model_resign_selfplay()
    print("resign:", want["outcomes"], want["stats"], want["resign_stats"])
    assert [(g, o.result, o.how) for _, g, o in want["outcomes"]] == [(0, "red", "mate"), (1, "black", "resign")]
    assert_selfplay(device_selfplay(*RESIGN_OPENINGS, 3, max_plies=8, rules="xiangqi", resign=2.0, resign_playon=0.0, seed=1), want,
                    XQ + ("resigned",))

    want = model_verdict_selfplay()
    print("verdict:", want["outcomes"], want["stats"])
    assert [(o.result, o.how, o.fin_n) for _, _, o in want["outcomes"]] == [("red", "perpetual", 1)]
    assert_selfplay(device_selfplay(MATES[None], np.array([1], np.uint8), None, 2, ring=mate_key(), max_plies=8, rules="xiangqi", repetition=2),
                    want, XQ)
