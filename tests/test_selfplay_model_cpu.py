"""The host model of the self-play kernels (tests/selfplay_model.py) against numpy and the golden self-play games.

choose_ref must be np.random.choice itself when handed the uniform choice would draw, and with the golden games' own numpy
streams it must reproduce every move the reference played, with margins large enough that the float32 uniforms the kernel
takes cannot change a pick (the GPU replay in test_selfplay_kernels.py rests on that).  adjudicate_ref must reproduce the
result and z of every golden game; flush_ref the ring arithmetic of k_sp_flush.
"""
import numpy as np
import pytest

import selfplay_model as M

START_FEN = "RNBAKABNR/9/1C5C1/P1P1P1P1P/9/9/p1p1p1p1p/1c5c1/9/rnbakabnr"


@pytest.mark.parametrize("temperature", [1.0, 0.5, 1e-3])
@pytest.mark.parametrize("eps", [0.0, 0.25])
def test_choose_ref_is_numpy_choice(temperature, eps):
    rng = np.random.default_rng(int(temperature * 1000) + int(eps * 100))
    for trial in range(300):
        k = int(rng.integers(1, 129))
        visits = rng.integers(0, 40, k)
        visits[rng.random(k) < 0.3] = 0
        if not visits.any():
            visits[int(rng.integers(k))] = 1      # the reference raises on all-zero visits: the departure is tested below
        gamma = rng.gamma(0.3, size=k)
        seed = int(rng.integers(1 << 31))
        p = 0.75 * M.visit_probs(visits, temperature) + 0.25 * (gamma / gamma.sum()) if eps else M.visit_probs(visits, temperature)
        want = np.random.RandomState(seed).choice(k, p=p)
        u = np.random.RandomState(seed).random_sample()
        got, margin = M.choose_ref(visits, temperature, gamma, eps, u)
        assert got == want, (trial, k)
        assert margin > 0


def test_choose_ref_departures_and_edges():
    # all visits zero: uniform over the children
    for u, want in ((0.0, 0), (0.2499, 0), (0.25, 1), (0.99, 3)):
        assert M.choose_ref([0, 0, 0, 0], 1.0, None, 0.0, u)[0] == want
    # gamma summing to zero over the children: no noise, whatever eps is
    assert M.choose_ref([1, 3], 1.0, [0.0, 0.0, 5.0], 1.0, 0.3)[0] == 1
    assert M.choose_ref([1, 3], 1.0, [0.0, 1.0], 1.0, 0.0)[0] == 1
    # eps = 1: only gamma counts; zero-probability children are skipped, u = 0 picks the first positive one
    assert M.choose_ref([5, 5, 5], 1.0, [0.0, 0.0, 2.0], 1.0, 0.0) == (2, np.inf)
    # u at the top of the range and past it (the rounding fallback: the last child with a positive probability)
    top = float(np.nextafter(np.float32(1), np.float32(0)))
    assert M.choose_ref([4, 2, 0], 1.0, None, 0.0, top)[0] == 1
    assert M.choose_ref([4, 2, 0], 1.0, None, 0.0, 1.0) == (1, np.inf)
    # temperature: 1e-3 sends the mass to the most visited child
    assert M.choose_ref([3, 9, 8], 1e-3, None, 0.0, 0.5)[0] == 1
    assert M.choose_ref([3, 9, 8], 1.0, None, 0.0, 0.5)[0] == 1
    assert M.choose_ref([3, 9, 8], 1.0, None, 0.0, 0.1)[0] == 0


def test_golden_stream_replays_every_reference_move():
    """np.random.seed(meta.seed) + per ply dirichlet(0.3 * ones(k)) and the uniform of np.random.choice: choose_ref with the
    float32-rounded uniform and the float32-rounded Dirichlet vector (what the kernel is handed) plays every golden move."""
    worst = np.inf
    for c in M.golden_games():
        stream = M.golden_stream(c["meta"]["seed"], c["count"])
        for ply, (d, u) in enumerate(stream):
            k = int(c["count"][ply])
            for gam, uu in ((d, u), (d.astype(np.float32), float(np.float32(u)))):
                pick, margin = M.choose_ref(c["visits"][ply, :k], 1.0, gam, 0.25, uu)
                assert int(c["labels"][ply, pick]) == int(c["played"][ply]), (c["meta"]["name"], ply)
                worst = min(worst, margin)
    assert worst >= 1e-9, worst


def test_adjudicate_ref_reproduces_every_golden_result():
    """The golden games replayed on the oracle's boards: adjudicate_ref finds no end before the last ply, and at the last one
    the reference's z; the statistics follow."""
    from oracle import oracle as O
    outcomes = []
    for c in M.golden_games():
        m = c["meta"]
        n = m["plies"]
        board, adj = M.replay_golden(c)
        assert np.array_equal(board[0], O.fen_to_board(START_FEN)) and np.array_equal(c["side"], np.arange(n) % 2)
        assert all(a is None for a in adj[:-1]), m["name"]
        out = adj[-1]
        assert out is not None and out.fin_n == n
        assert np.array_equal(out.z.astype(np.float64), c["z"]), m["name"]
        assert (out.result == "draw") == (m["z_first"] == 0)
        outcomes.append(out)
    st = M.stats_ref(outcomes)
    assert st["games"] == 6 and st["plies"] == 342 and st["stalled"] == 0
    assert st["draws"] == 1 and st["red_wins"] + st["black_wins"] == 5


def test_adjudicate_ref_extensions():
    from oracle import oracle as O
    b = O.fen_to_board(START_FEN)
    movers = [0, 1, 0, 1, 0]
    assert M.adjudicate_ref(b, 10, 5, movers, 512) is None
    o = M.adjudicate_ref(b, 10, 5, movers, 5)                      # the history is full: a draw with every record
    assert o.result == "draw" and o.fin_n == 5 and not o.z.any()
    o = M.adjudicate_ref(b, 10, 7, movers + [1, 0], 5)             # more plies than the history holds: fin_n = max_plies
    assert o.fin_n == 5 and len(o.z) == 5
    assert M.adjudicate_ref(b, 59, 5, movers, 512) is None
    assert M.adjudicate_ref(b, 60, 5, movers, 512).result == "draw"
    o = M.adjudicate_ref(b, 3, 5, movers, 512, stalled=True)
    assert o.result == "stalled" and o.fin_n == 0
    nok = b.copy()
    nok[nok == M.KING_BLACK] = 0                                   # 'k' gone: red wins, even at rr >= 60
    o = M.adjudicate_ref(nok, 60, 5, movers, 512)
    assert o.result == "red" and list(o.z) == [1, -1, 1, -1, 1]
    noK = b.copy()
    noK[noK == M.KING_RED] = 0
    o = M.adjudicate_ref(noK, 0, 4, movers[:4], 512)
    assert o.result == "black" and list(o.z) == [-1, 1, -1, 1]
    assert M.stats_ref([o, M.adjudicate_ref(b, 60, 1, [0], 9)]) == dict(games=2, red_wins=0, black_wins=1, draws=1, plies=5, stalled=0)


def test_flush_ref_wraps_and_drops_whole_games():
    R, B = 7, 4
    hist = [np.full((5, B), 10 * (g + 1) + np.arange(5)[:, None], np.uint8) for g in range(3)]
    ring = np.full((R, B), 0xEE, np.uint8)
    fin_n = [3, 0, 4]
    offset = [5, 8, 8]
    out, dropped = M.flush_ref(ring, hist, fin_n, offset)
    assert dropped == 0
    want = ring.copy()
    for g in (0, 2):
        for j in range(fin_n[g]):
            want[(offset[g] + j) % R] = hist[g][j]
    assert np.array_equal(out, want)
    # read_cursor 5: rows up to 5 + 7 = 12 may be written: game 0 (5..7) is, game 2 (8..11) ends exactly there and is too
    out, dropped = M.flush_ref(ring, hist, fin_n, offset, read_cursor=5)
    assert dropped == 0 and np.array_equal(out, want)
    # read_cursor 4: game 2 would pass 11 -> dropped whole, its rows keep what they held
    out, dropped = M.flush_ref(ring, hist, fin_n, offset, read_cursor=4)
    assert dropped == 4
    assert np.array_equal(out[[5, 6, 0]], hist[0][:3]) and (out[[1, 2, 3, 4]] == 0xEE).all()
