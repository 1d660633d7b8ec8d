"""Evaluation matches without a GPU: the score / Elo / pentanomial arithmetic of cchess_zero_amd/arena.py, the host model of
the match kernels (tests/match_model.py: two oracle.Search players per game), the rank-sharding merge under gloo, and the
command lines (main.py --eval_every, python -m cchess_zero_amd.arena)."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import fakenet
import match_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _openings(n, plies, seed):
    """n distinct positions after `plies` random legal plies (oracle rules), both kings present."""
    from oracle import oracle as O
    from cchess_zero_amd.arena import Openings
    rng = np.random.RandomState(seed)
    out, keys = [], set()
    while len(out) < n:
        b, s, rr, ok = O.fen_to_board(O.START_FEN), 0, 0, True
        for _ in range(plies):
            mv = O.legal_moves(b, s)
            b, cap, term = O.apply_move(b, int(mv[rng.randint(len(mv))]))
            rr = 0 if cap else rr + 1
            s ^= 1
            ok = ok and not term
        k = O.zhash(b, s)
        if ok and k not in keys:
            keys.add(k)
            out.append((b, s, rr))
    return Openings(np.stack([o[0] for o in out]), [o[1] for o in out], [o[2] for o in out])


def _players(pa=8, pb=6):
    return [(fakenet.make_forward("pos", 11), pa), (fakenet.make_forward("signed", 12), pb)]


# ---- arithmetic ------------------------------------------------------------------------------------------------------------
def test_elo_of_even_score_is_zero_and_all_wins_is_infinite():
    from cchess_zero_amd.arena import MatchResult, elo
    assert elo(0.5) == 0.0
    assert elo(0.75) == pytest.approx(400 * math.log10(3))
    # every scored game won (or lost): the difference is infinite, reported as None
    assert elo(1.0) is None and elo(0.0) is None and elo(None) is None
    n = 4
    r = MatchResult(np.ones(n), [1, 0, 1, 0], np.full(n, 10), np.full(n, MM.KING), None, 0, 1.0, [])
    assert r.score == 1.0 and r.elo is None and r.to_dict()["elo"] is None
    assert r.elo_95 == (None, None)   # zero variance: the interval collapses onto the infinite point
    # aborted games are not scored
    r = MatchResult([1, -1, 0, 0], [1, 0, 1, 0], [5, 5, 5, 5], [MM.KING, MM.KING, MM.ABORTED, MM.RR60], None, 0, 1.0, [])
    assert (r.wins, r.draws, r.losses, r.aborted, r.scored) == (1, 1, 1, 1, 3) and r.score == pytest.approx(0.5)
    assert r.by_colour == {"red": {"W": 1, "D": 0, "L": 0}, "black": {"W": 0, "D": 1, "L": 1}}


def test_pentanomial_by_hand():
    from cchess_zero_amd.arena import MatchResult, elo, pentanomial, pentanomial_interval
    # pairs: (win, win) = 2 points, (win, loss) = 1, (draw, draw) = 1, (loss, draw) = 0.5; pair 4 has an aborted game
    result = [1, 1, 1, -1, 0, 0, -1, 0, 1, 0]
    reason = [MM.KING, MM.KING, MM.KING, MM.KING, MM.RR60, MM.PLY_CAP, MM.KING, MM.RR60, MM.KING, MM.ABORTED]
    c = pentanomial(result, reason)
    assert c.tolist() == [0, 1, 2, 0, 1]
    s, lo, hi = pentanomial_interval(c)
    # per-game pair scores 1.0, 0.5, 0.5, 0.25: mean 0.5625, variance ((0.4375)^2 + 2 (0.0625)^2 + (0.3125)^2) / 4
    var = (0.4375 ** 2 + 2 * 0.0625 ** 2 + 0.3125 ** 2) / 4
    assert s == pytest.approx(0.5625)
    assert hi - s == pytest.approx(1.959963984540054 * math.sqrt(var / 4)) and s - lo == pytest.approx(hi - s)
    r = MatchResult(result, [1, 0] * 5, [9] * 10, reason, None, 0, 1.0, [])
    assert r.pentanomial.tolist() == [0, 1, 2, 0, 1]
    assert r.elo_95[0] == pytest.approx(elo(lo)) and r.elo_95[1] == pytest.approx(elo(hi))
    # an interval past 1: unbounded above
    s, lo, hi = pentanomial_interval([0, 0, 1, 0, 1])
    assert (s, round(lo, 6)) == (0.75, round(0.75 - 1.959963984540054 * math.sqrt(0.0625 / 2), 6)) and hi > 1
    assert pentanomial_interval([0, 0, 0, 0, 0]) is None


def test_uniform_is_a_pure_function_of_seed_game_and_ply():
    us = [MM.uniform(7, g, p) for g in range(50) for p in range(20)]
    assert all(0.0 <= u < 1.0 for u in us) and len(set(us)) == len(us)
    assert MM.uniform(7, 3, 4) == MM.uniform(7, 3, 4) != MM.uniform(8, 3, 4)
    # splitmix64 reference values (the published finaliser from state 0 and 1)
    assert MM.splitmix64(0) == 0xE220A8397B1DCDAF   # the first output of SplitMix64 from state 0


def test_choose_greedy_takes_the_first_maximum_and_sampling_follows_the_cdf():
    assert MM.choose([3, 5, 5, 1], ply=9, sample_plies=2, seed=0, game=0) == 1
    assert MM.choose([0, 0, 0], ply=0, sample_plies=0, seed=0, game=0) == 0
    # sampled: frequencies of softmax(log N) = N / sum N over many games
    N = np.array([1, 3, 0, 6])
    picks = np.bincount([MM.choose(N, 0, 1, 5, g) for g in range(4000)], minlength=4)
    assert picks[2] == 0 and np.allclose(picks / 4000, N / N.sum(), atol=0.03)


def test_queue_order():
    op, a_red, first = MM.queue(3, 8)
    assert op.tolist() == [0, 0, 1, 1, 2, 2] and a_red.tolist() == [1, 0, 1, 0, 1, 0]
    assert first.tolist() == [0, 1, 2, 3, 4, 5, -1, -1]


# ---- model matches ---------------------------------------------------------------------------------------------------------
def test_model_match_is_colour_symmetric_when_a_equals_b():
    op = _openings(3, 4, seed=1)
    p = (fakenet.make_forward("pos", 11), 8)
    m = MM.play_match([p, p], op, max_plies=40)
    for k in range(3):
        assert m["moves"][2 * k].tolist() == m["moves"][2 * k + 1].tolist()
        assert m["a_red"][2 * k] == 1 and m["a_red"][2 * k + 1] == 0
        assert m["result"][2 * k] == -m["result"][2 * k + 1] and m["reason"][2 * k] == m["reason"][2 * k + 1]
    from cchess_zero_amd.arena import MatchResult
    r = MatchResult(m["result"], m["a_red"], m["plies"], m["reason"], m["moves"], 0, 1.0, [])
    assert r.score == 0.5 and r.elo == 0.0


def test_swapping_a_and_b_negates_every_result():
    op = _openings(3, 4, seed=2)
    pa, pb = _players()
    ab = MM.play_match([pa, pb], op, max_plies=40)
    ba = MM.play_match([pb, pa], op, max_plies=40)
    # game 2p of one match is game 2p + 1 of the other with the players' names swapped: the same player has the same
    # colour, so it is the same game move for move, and A's result is the other one's
    swap = np.arange(6) ^ 1
    assert np.array_equal(ba["moves"], ab["moves"][swap]) and np.array_equal(ba["reason"], ab["reason"][swap])
    assert np.array_equal(ba["result"], -ab["result"][swap])
    assert ab["reason"].min() >= MM.KING


# ---- ranks ---------------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cchess_zero_amd import arena
    op = _openings(5, 4, seed=3)
    mine = arena.rank_pairs(5, rank, world)
    local = MM.play_match(_players(), op, max_plies=30, sample_plies=2, seed=4, pairs=mine)
    local.update(simulations=100 * (rank + 1), seconds=1.0 + rank)
    merged = arena.merge_ranks(local, 5, rank, world)
    q.put((rank, mine.tolist(), {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in merged.items()}))
    dist.monitored_barrier()
    dist.destroy_process_group()


def test_rank_sharding_merge_gloo_world2_equals_world1():
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, mine0, m0), (r1, mine1, m1) = res
    assert mine0 == [0, 2, 4] and mine1 == [1, 3]
    assert m0 == m1
    one = MM.play_match(_players(), _openings(5, 4, seed=3), max_plies=30, sample_plies=2, seed=4)
    for k in ("result", "a_red", "plies", "reason", "moves"):
        assert m0[k] == one[k].tolist(), k
    assert m0["simulations"] == 300 and m0["seconds"] == 2.0


# ---- command lines -------------------------------------------------------------------------------------------------------
def _help(args):
    p = subprocess.run([sys.executable] + args + ["--help"], capture_output=True, text=True, cwd=ROOT, timeout=300,
                       stdin=subprocess.DEVNULL)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_main_help_lists_eval_flags_and_keeps_modes():
    out = _help([os.path.join(ROOT, "main.py")])
    assert "--eval_every" in out and "--eval_games" in out and "{train,play}" in out


def test_arena_module_help_runs():
    out = _help(["-m", "cchess_zero_amd.arena"])
    for flag in ("--a", "--b", "--blocks", "--games", "--playout", "--playout_b", "--opening_plies", "--slots", "--seed"):
        assert flag in out
