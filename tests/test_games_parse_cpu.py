"""cchess_zero_amd/games.py without a GPU: the parser and the writer of the two text formats (round trip, malformed input), and
pretrain's batches with a recording fake net on the model's records of the reference's six games: the documented draw, the
holdout by game, the mirror coins and the holdout figures."""
import math
import random

import numpy as np
import pytest

import games_model as GM


def _golden_as_games():
    from cchess_zero_amd import games as GG
    moves, lens, results, _, _ = GM.golden_games()
    return GG.games_from_labels(moves, lens, results)


def test_round_trip_in_both_formats():
    from cchess_zero_amd import games as GG
    from cchess_zero_amd.notation import fen_to_position
    gs = _golden_as_games()
    gs[3] = gs[3]._replace(result=None)
    assert GG.parse_games(GG.write_games(gs, pgn=False)) == gs
    b, s, rr = fen_to_position("3k5/9/9/9/4r4/9/9/9/4R4/4K4 b - - 7 1")
    l2i = {n: i for i, n in enumerate(__import__("oracle.oracle", fromlist=["x"]).labels())}
    gs.append(GG.Game(bytes(b), s, rr, (l2i["e5e1"], l2i["e0e1"], l2i["d9d8"]), 0, (("Event", "a constructed game"), ("Red", "somebody"))))
    gs.append(GG.Game(bytes(b), 0, 0, (), None, ()))
    text = GG.write_games(gs, pgn=True)
    back = GG.parse_games(text)
    assert back == gs and back.skipped == ()
    assert "1. ... E5-E1 2. E0-E1 D9-D8" in text and '[FEN "3k5/9/9/9/4r4/9/9/9/4R4/4K4 b - - 7 1"]' in text
    with pytest.raises(ValueError):
        GG.write_games(gs, pgn=False)          # a start position has no place on a line


def test_what_the_parser_reads():
    from cchess_zero_amd import games as GG
    from cchess_zero_amd._lib import tables
    l2i = tables()["label2i"]
    g = GG.parse_games("h2e2 h9g7 1-0\n\n# a comment\nH2-E2 h9-g7 h0g2 0-1\nb0c2 *\nb0c2 1/2-1/2\n")
    assert [x.labels for x in g] == [(l2i["h2e2"], l2i["h9g7"]), (l2i["h2e2"], l2i["h9g7"], l2i["h0g2"]), (l2i["b0c2"],), (l2i["b0c2"],)]
    assert [x.result for x in g] == [1, -1, None, 0] and g.skipped == ()
    p = GG.parse_games('[Event "x"]\n[Result "0-1"]\n\n1. H2-E2 {the central cannon\n over two lines} H9-G7\n2. h0g2 0-1\n\n[Result "*"]\n1.b0c2 *\n')
    assert [x.labels for x in p] == [(l2i["h2e2"], l2i["h9g7"], l2i["h0g2"]), (l2i["b0c2"],)] and [x.result for x in p] == [-1, None]
    assert p[0].tags == (("Event", "x"),) and p[1].tags == ()


def test_malformed_input_is_reported_and_skipped_never_guessed():
    from cchess_zero_amd import games as GG
    g = GG.parse_games("h2e2 h9g7 1-0\nh2e2 z9g7 1-0\nh2e2 a0b5\nh2e2\n")
    assert len(g) == 2 and [s[0] for s in g.skipped] == [2, 3] and "z9g7" in g.skipped[0][1] and "a0b5" in g.skipped[1][1]
    text = ('[Format "WXF"]\n[Result "1-0"]\n1. C2=5 H8+7 1-0\n\n'           # says it is not ICCS
            '[Result "1-0"]\n1. C2=5 H8+7 1-0\n\n'                             # does not say so, but is not
            '[FEN "9/9/9/9/9/9/9/9/9/4K4 w"]\n[Result "1-0"]\n1. E0-E1 1-0\n\n'   # a FEN without the black king
            '[Result "2-0"]\n1. H2-E2\n\n'                                     # no such result
            '[Result "1-0"]\n1. H2-E2 {never closed\n\n'
            '[Result "1/2-1/2"]\n1. H2-E2 1/2-1/2\n')
    p = GG.parse_games(text)
    assert len(p) == 1 and p[0].result == 0 and len(p.skipped) == 5
    why = " | ".join(s[1] for s in p.skipped)
    assert "WXF" in why and "C2=5" in why and "king" in why and "2-0" in why and "comment" in why


class FakeNet:
    """records what it is trained on; forward answers a fixed function of the planes"""

    def __init__(self):
        self.calls, self.global_step = [], 0

    def train_step(self, planes, pi, z, lr):
        self.calls.append((np.asarray(planes), np.asarray(pi), np.asarray(z), lr))
        self.global_step += 1
        return 0.5, 10.0 - len(self.calls), self.global_step

    def forward(self, planes):
        x = np.asarray(planes, np.float64).reshape(len(planes), -1)
        logits = np.zeros((len(x), 2086))
        for c in range(14):
            logits[:, 37 * c:37 * c + 1260 // 14 * 2] += x[:, c::14].sum(axis=1, keepdims=True) * np.cos(np.arange(180) * (c + 1))[None, :]
        logits[:, 600:1860] += x[:, :1260] * 3.0
        return logits.astype(np.float32), (x[:, ::7].sum(axis=1) % 3 - 1).astype(np.float32).reshape(-1, 1)


@pytest.fixture(scope="module")
def model_records():
    moves, lens, results, _, _ = GM.golden_games()
    out = GM.replay(None, None, moves, lens, results, 0)
    return out["records"], np.repeat(np.arange(6), lens).astype(np.int32)


@pytest.mark.parametrize("mirror", [False, True])
def test_pretrain_trains_on_the_documented_draw(model_records, mirror):
    from cchess_zero_amd import games as GG
    from cchess_zero_amd.records import mirror_records
    from cchess_zero_amd.selfplay import to_dense
    rec, game_of = model_records
    seed, steps, B, holdout = 11, 4, 16, 0.3
    net = FakeNet()
    info = GG.pretrain(net, rec, game_of, steps, B, 0.01, seed, mirror=mirror, holdout=holdout, log=lambda *_: None)
    ids = list(range(6))
    random.Random(seed).shuffle(ids)
    held = ids[6 - math.ceil(0.3 * 6):]
    assert len(held) == 2 and info["holdout_games"] == 2
    train_idx = np.nonzero(~np.isin(game_of, held))[0]
    hold_idx = np.nonzero(np.isin(game_of, held))[0]
    assert info["train_records"] == len(train_idx) and info["holdout_records"] == len(hold_idx) and len(net.calls) == steps
    coins_total = 0
    for s, (planes, pi, z, lr) in enumerate(net.calls):
        rng = random.Random((seed << 32) ^ s)
        idx = train_idx[rng.sample(range(len(train_idx)), B)]
        assert not np.isin(game_of[idx], held).any()
        r = rec[idx]
        if mirror:
            coins = np.array([rng.getrandbits(1) for _ in idx], np.uint8)
            coins_total += int(coins.sum())
            r = mirror_records(r, coins)
        want = to_dense(r, 1.0, exact=True)
        assert np.array_equal(planes, want[0]) and np.array_equal(pi, want[1]) and np.array_equal(z.reshape(-1), want[2]) and lr == 0.01
    assert info["mirrored"] == coins_total and (not mirror or 0 < coins_total < steps * B)
    assert info["losses"] == [9.0, 8.0, 7.0, 6.0]
    # the holdout figures, computed directly
    planes, pi, z = to_dense(rec[hold_idx], 1.0, exact=True)
    logits, v = net.forward(list(planes))
    logits = logits.astype(np.float64)
    played = pi.argmax(axis=1)
    logp = logits - np.log(np.exp(logits - logits.max(axis=1, keepdims=True)).sum(axis=1, keepdims=True)) - logits.max(axis=1, keepdims=True)
    assert info["top1"] == float((logits.argmax(axis=1) == played).mean())
    assert abs(info["logloss"] - float(-logp[np.arange(len(played)), played].mean())) < 1e-9
    assert info["value_sign"] == float((np.sign(v.reshape(-1)) == np.sign(z)).mean())


def test_pretrain_without_holdout_and_with_a_small_buffer(model_records):
    from cchess_zero_amd import games as GG
    rec, game_of = model_records
    net = FakeNet()
    info = GG.pretrain(net, rec[:5], game_of[:5], 2, 64, 0.1, 3, holdout=0, log=lambda *_: None)
    assert info["holdout_records"] == 0 and info["top1"] is None and info["train_records"] == 5
    assert all(len(c[0]) == 5 for c in net.calls)          # min(batch_size, training records), drawn without replacement
    with pytest.raises(ValueError):
        GG.pretrain(net, rec[:5], game_of[:5], 1, 4, 0.1, 3, holdout=1.0, log=lambda *_: None)


def test_infer_result():
    from cchess_zero_amd import games as GG
    assert GG.infer_result(16, 0) == -1 and GG.infer_result(32 | 2, 1) == 1 and GG.infer_result(4 | 1, 0) == -1 and GG.infer_result(4, 1) == 1
    assert GG.infer_result(1, 0) is None and GG.infer_result(0, 1) is None
