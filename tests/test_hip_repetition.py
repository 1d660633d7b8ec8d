"""cz_repetition (csrc/cz_repetition.hip, Rules.repetition) against tests/repetition_model.py, bit for bit in verdict and first,
on random histories that repeat often and cross the kernel's 64-position chunks."""
import itertools

import numpy as np
import pytest
import torch

import repetition_model as RM

pytestmark = pytest.mark.gpu

STRIDE = 208                                           # > every length: the rows end in garbage that must not be read
LENGTHS = (1, 2, 5, 9, 63, 64, 65, 129, 200)           # around the chunk boundaries at 64 and 128 earlier positions
WINDOWS = ("null", "zero", "all", "random")


@pytest.fixture(scope="module")
def launches():
    """One entry per launch: every (G, fold, window kind) — 16 x (1 + 3 + 64 + 67) = 2 160 games — and eight launches of
    far-reaching cycles, with the model's answers."""
    rng = np.random.default_rng(2025)
    out, k = [], 0
    shapes = [(G, fold, wk, False) for G, fold, wk in itertools.product((1, 3, 64, 67), (2, 3, 4, 8), WINDOWS)]
    # and, beyond those: histories whose only repetitions are fold - 1 planted ones anywhere in the game, so that the cycle often
    # starts two or three chunks back (six key values repeat within a few plies)
    shapes += [(67, fold, wk, True) for fold, wk in itertools.product((2, 3, 4, 8), ("null", "random"))]
    for G, fold, wk, far in shapes:
        keys = rng.integers(0, 6, (G, STRIDE)).astype(np.uint64) ^ rng.integers(0, 1 << 63, (G, 1)).astype(np.uint64)
        checks = (rng.random((G, STRIDE)) < 0.5).astype(np.uint8)
        length = np.zeros(G, np.int32)
        for g in range(G):
            length[g] = LENGTHS[k % len(LENGTHS)]
            k += 1
            if far:
                n = int(length[g]) - 1
                keys[g] = np.arange(STRIDE, dtype=np.uint64) + np.uint64(1000 * g)
                if n >= fold - 1:
                    keys[g, rng.choice(n, fold - 1, replace=False)] = keys[g, n]
            if rng.random() < 0.5:                       # one side checks with every move, the other now and then
                par = int(rng.integers(2))
                checks[g, par::2] = 1
                checks[g, 1 - par::2] = rng.random(len(checks[g, 1 - par::2])) < 0.3
        side = rng.integers(0, 2, G).astype(np.uint8)
        window = {"null": None, "zero": np.zeros(G, np.int32), "all": length - 1,
                  "random": np.array([rng.integers(-2, n + 3) for n in length], np.int32)}[wk]
        want = [RM.verdict(keys[g, :length[g]].tolist(), checks[g, :length[g]].tolist(), int(side[g]),
                           None if window is None else int(window[g]), fold) for g in range(G)]
        out.append(dict(G=G, fold=fold, keys=keys, checks=checks, length=length, side=side, window=window,
                        verdict=np.array([w[0] for w in want], np.uint8), first=np.array([w[1] for w in want], np.int32)))
    return out


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


def test_the_model_answers_every_verdict_often(launches):
    assert sum(c["G"] for c in launches) >= 2000
    v = np.concatenate([c["verdict"] for c in launches])
    counts = np.bincount(v, minlength=4)
    assert len(counts) == 4 and (counts >= 50).all(), counts
    f = np.concatenate([c["first"] for c in launches])
    n = np.concatenate([c["length"] for c in launches]) - 1
    assert ((f >= 0) == (v != RM.NONE)).all()
    assert (n - f > 64)[v != RM.NONE].sum() >= 20 and (n - f > 128)[v != RM.NONE].sum() >= 5   # cycles found in a later chunk


def test_cz_repetition_equals_the_model(rules, launches):
    for c in launches:
        verdict, first = rules.repetition(c["keys"].view(np.int64), c["checks"], c["side"], c["length"], c["window"], c["fold"])
        tag = (c["G"], c["fold"], None if c["window"] is None else c["window"][:4])
        assert np.array_equal(verdict.cpu().numpy(), c["verdict"]), tag
        assert np.array_equal(first.cpu().numpy(), c["first"]), tag


def test_default_length_and_null_first(rules, launches):
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import _ptr
    c = launches[63]                                     # G = 67, fold 8, six key values
    G = c["G"]
    want = [RM.verdict(c["keys"][g].tolist(), c["checks"][g].tolist(), int(c["side"][g]), None, 3) for g in range(G)]
    verdict, first = rules.repetition(c["keys"].view(np.int64), c["checks"], c["side"])          # the whole row, fold 3
    assert verdict.cpu().numpy().tolist() == [w[0] for w in want] and first.cpu().numpy().tolist() == [w[1] for w in want]
    assert (np.array([w[0] for w in want]) != RM.NONE).any()
    keys, checks = torch.from_numpy(c["keys"].view(np.int64)).cuda(), torch.from_numpy(c["checks"]).cuda()
    side, length = torch.from_numpy(c["side"]).cuda(), torch.full((G,), STRIDE, dtype=torch.int32, device="cuda")
    out = torch.full((G,), 99, dtype=torch.uint8, device="cuda")
    rules.ctx.bind_stream()
    check(lib().cz_repetition(rules.ctx.h, _ptr(keys), _ptr(checks), STRIDE, _ptr(length), None, _ptr(side), G, 3, _ptr(out), None), "cz_repetition")
    assert out.cpu().numpy().tolist() == [w[0] for w in want]
    # a length outside the row answers "no verdict" and reads nothing
    bad = torch.tensor([0, STRIDE + 1, -5], dtype=torch.int32, device="cuda")
    verdict, first = rules.repetition(c["keys"][:3].view(np.int64), c["checks"][:3], c["side"][:3], bad, None, 2)
    assert verdict.cpu().numpy().tolist() == [0, 0, 0] and first.cpu().numpy().tolist() == [-1, -1, -1]


def test_bad_arguments_are_einval(rules):
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd.engine import _ptr
    keys = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    checks = torch.zeros((2, 4), dtype=torch.uint8, device="cuda")
    side = torch.zeros(2, dtype=torch.uint8, device="cuda")
    length = torch.full((2,), 4, dtype=torch.int32, device="cuda")
    verdict = torch.zeros(2, dtype=torch.uint8, device="cuda")
    L, h = lib(), rules.ctx.h

    def call(keys_=keys, stride=4, fold=3, G=2, verdict_=verdict, length_=length, h_=h):
        return L.cz_repetition(h_, _ptr(keys_), _ptr(checks), stride, _ptr(length_), None, _ptr(side), G, fold, _ptr(verdict_), None)
    assert call() == 0
    for kw in (dict(fold=1), dict(fold=9), dict(fold=0), dict(keys_=None), dict(stride=0), dict(G=-1), dict(verdict_=None),
               dict(length_=None), dict(h_=None)):
        assert call(**kw) == -1, kw                      # CZ_EINVAL
        assert L.cz_last_error()
    assert call(G=0) == 0
