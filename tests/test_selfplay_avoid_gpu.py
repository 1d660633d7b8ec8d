"""Self-play with the avoid step (cz_selfplay_set_avoid, SelfPlay(avoid_repetition=True)): whole games, records and pi included,
equal tests/avoid_model.py's replay of tests/selfplay_rules_model.py's loop byte for byte; the constructed perpetual check is not
played into; off is self-play as it was; the setter keeps its order."""
import numpy as np
import pytest

import avoid_model as AM
import fakenet
import match_model as MM
import repetition_cases as RC
import selfplay_rules_model as XS
from test_selfplay_rules_gpu import STATS, XQ_STATS, _selfplay

pytestmark = pytest.mark.gpu
EINVAL = -1


def _stream(G, T):
    rng = np.random.default_rng(1)
    stream = [(rng.gamma(0.3, size=(G, 128)).astype(np.float32), rng.random(G).astype(np.float32)) for _ in range(T)]
    for gamma, _ in stream:
        gamma[8:] = 0
    return stream


def _run(boards, side, playouts, stream, fwd, **kw):
    eng, sp = _selfplay(boards, side, playouts, cap=1 << 15, continuous=False, rules="xiangqi", repetition=3, **kw)
    for rand in stream:
        sp.step_ply(fwd, rand=rand)
    return sp, sp.drain(), sp.stats()


def _same(rec, st, sp, ref):
    assert {k: st[k] for k in STATS + XQ_STATS} == {k: ref["stats"][k] for k in STATS + XQ_STATS} and st["dropped"] == 0
    assert np.array_equal(sp.active().numpy().astype(bool), ref["active"])
    assert rec.shape == ref["records"].shape and np.array_equal(rec, ref["records"])


def test_games_from_openings_with_the_avoid_step_equal_the_model():
    """Six CPU-made openings, 8 playouts, 24 lock-step plies at temperature 0.05 with max_plies 20, slots 0-2 with Dirichlet noise, at
    the chase level: records, pi and counters equal the model whether the step finds something to remove or not."""
    G, T, playouts, max_plies, temperature = 6, 24, 8, 20, 0.05
    boards, side = RC.cpu_openings(G, 4, 11)
    stream = _stream(G, T)
    for gamma, _ in stream:
        gamma[3:] = 0
    with AM.avoiding() as counters:
        want = XS.play_games(fakenet.make_forward("pos", 11), playouts, boards, side, None, stream, max_plies=max_plies, temperature=temperature,
                             fold=3, chase=True)
    print("model:", want["stats"], counters, "min margin %.3g" % want["min_margin"])
    assert want["min_margin"] >= 1e-12 and not want["active"].any()
    sp, rec, st = _run(boards, side, playouts, stream, MM.device_forward("pos", 11), exploration=True, temperature=temperature, max_plies=max_plies,
                       chase=True, avoid_repetition=True)
    _same(rec, st, sp, want)
    assert (st["avoided"], st["forced_repetitions"]) == (counters["avoided"], counters["forced_repetitions"])


def test_the_constructed_perpetual_check_is_not_played_into():
    """Two slots on the constructed position under the steering net, greedy: without the step red loses at ply 8 by perpetual check
    and that z goes into eight records; with it red leaves the line at ply 6, and every record and pi equals the model's."""
    b = RC.perpetual_board()
    T = 14
    stream = [(None, np.full(2, 0.5, np.float32)) for _ in range(T)]
    kw = dict(max_plies=12, temperature=0.05, eps=0.0, fold=3)
    plain = XS.play_games(RC.steering_forward(), RC.PERPETUAL_PLAYOUTS, [b, b], [0, 0], None, stream, **kw)
    assert [(t, o.how) for t, _, o in plain["outcomes"]] == [(8, "perpetual")] * 2               # red loses at ply 8
    with AM.avoiding() as counters:
        want = XS.play_games(RC.steering_forward(), RC.PERPETUAL_PLAYOUTS, [b, b], [0, 0], None, stream, **kw)
    print("model:", want["stats"], counters, [(t, o.how) for t, _, o in want["outcomes"]])
    assert counters["avoided"] >= 2 and want["stats"]["perpetuals"] == 0 and want["stats"]["games"] == 2
    fwd = RC.steering_device_forward()
    sp, rec, st = _run([b, b], [0, 0], RC.PERPETUAL_PLAYOUTS, stream, fwd, exploration=False, temperature=0.05, max_plies=12, avoid_repetition=True)
    _same(rec, st, sp, want)
    assert st["avoided"] == counters["avoided"] and st["forced_repetitions"] == counters["forced_repetitions"]
    sp, rec, st = _run([b, b], [0, 0], RC.PERPETUAL_PLAYOUTS, stream, fwd, exploration=False, temperature=0.05, max_plies=12)
    _same(rec, st, sp, plain)                                                                     # off: self-play as it was
    assert "avoided" not in st and st["perpetuals"] == 2


def test_set_avoid_keeps_the_setters_order():
    from cchess_zero_amd._lib import lib
    L = lib()
    b = RC.perpetual_board()
    eng, sp = _selfplay([b], [0], 4, continuous=False, rules="xiangqi")
    h = eng.ctx.h
    assert L.cz_selfplay_set_avoid(None, 1) == EINVAL and L.cz_selfplay_avoid_stats(None, None) == EINVAL
    assert L.cz_selfplay_set_avoid(h, 1) == EINVAL                       # needs a fold
    assert L.cz_selfplay_set_repetition(h, 3) == 0 and L.cz_selfplay_set_avoid(h, 1) == 0
    assert L.cz_selfplay_set_repetition(h, 0) == EINVAL and L.cz_selfplay_set_avoid(h, 0) == 0 and L.cz_selfplay_set_repetition(h, 0) == 0
    sp.step_ply(MM.device_forward("pos", 11), rand=(None, np.full(1, 0.5, np.float32)))
    assert L.cz_selfplay_set_avoid(h, 1) == EINVAL
