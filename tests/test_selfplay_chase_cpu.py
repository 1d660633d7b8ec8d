"""tests/selfplay_rules_model.py with the perpetual-chase rule (self-play on the CPU oracle): the constructed chase as a forced
line — it ends at ply 8 as a loss for red, the chaser — and whole games in which every kind of ending occurs."""
import functools

import numpy as np

import chase_cases as CC
import fakenet
import repetition_cases as RC
import selfplay_rules_model as XS

# whole games: 16 openings, pos/11 at 16 playouts, 81 lock-step plies at temperature 0.01 without noise, max_plies 80
WHOLE = dict(G=16, T=81, playouts=16, max_plies=80, temperature=0.01)


def whole_games_stream():
    rng = np.random.default_rng(1)
    return [(None, rng.random(WHOLE["G"]).astype(np.float32)) for _ in range(WHOLE["T"])]


@functools.lru_cache(maxsize=None)
def whole_games_model(chase=True):
    """The whole games on the CPU oracle, once per process and setting; read-only."""
    boards, side = RC.cpu_openings(WHOLE["G"], 4, 11)
    return XS.play_games(fakenet.make_forward("pos", 11), WHOLE["playouts"], boards, side, None, whole_games_stream(),
                         max_plies=WHOLE["max_plies"], temperature=WHOLE["temperature"], eps=0.0, fold=3, chase=chase)


def test_the_constructed_chase_ends_at_ply_8_as_a_loss_for_red():
    line = [CC.label_of(m) for m in CC.CHASE_LINE] + [0xFFFF]
    forced = [np.array([l], np.uint16) for l in line]
    stream = [(None, np.full(1, 0.5, np.float32))] * 9
    for chase, how, z in ((True, "chase", [-1, 1] * 4), (False, "repetition", [0] * 8)):
        out = XS.play_games(fakenet.make_forward("pos", 11), 8, CC.CHASE_BOARD[None], [0], None, stream, max_plies=64, eps=0.0, fold=3,
                            forced=forced, chase=chase)
        (t, g, o), = out["outcomes"]
        assert (t, g, o.how, o.fin_n) == (8, 0, how, 8) and o.z.tolist() == z
        assert out["stats"]["chases"] == (1 if chase else 0) and out["stats"]["perpetuals"] == 0
        assert out["stats"]["black_wins"] == (1 if chase else 0) and out["stats"]["repetitions"] == (0 if chase else 1)
        assert len(out["records_chase"][0]) == 9


def test_whole_games_end_in_every_way():
    on, off = whole_games_model(), whole_games_model(chase=False)
    print("model:", on["stats"], "min margin %.3g over %d picks" % (on["min_margin"], on["picks"]))
    assert on["min_margin"] >= 1e-12 and not on["active"].any()
    assert on["stats"]["chases"] >= 1 and on["stats"]["repetitions"] >= 1 and on["stats"]["mates"] >= 1
    # without the rule the same games are played; a chase is a draw by repetition
    assert off["stats"]["chases"] == 0 and off["stats"]["repetitions"] == on["stats"]["repetitions"] + on["stats"]["chases"]
    assert off["records"].shape == on["records"].shape
    from cchess_zero_amd._lib import REC_Z
    same = np.delete(on["records"], REC_Z, axis=1) == np.delete(off["records"], REC_Z, axis=1)
    assert same.all()
