"""cz_threats (k_threats around cz_chase.h's czc_position) and cz_repetition_chase (wave_repetition_chase) on the GPU against
tests/chase_model.py, bit for bit: the table of constructed positions, random playouts, the golden rules positions, ragged batch
sizes at odd board addresses through the raw C ABI, refused boards; the verdict on the constructed chase and on 2 160 synthetic
game records whose chase records are real consecutive positions."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import chase_cases as CC
import chase_model as CM
import repetition_model as RM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _hold(rules, ref):
    boards, side, recs = ref
    got = _u64(rules.threats(boards.copy(), side.copy()))          # the shared reference is read-only
    bad = np.nonzero((got != recs).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], got[bad[:2]], recs[bad[:2]])
    return int(((recs[:, 0] | recs[:, 1]) != 0).sum())


def test_table(rules):
    _hold(rules, CM.table_reference())
    got = _u64(rules.threats(np.stack([c[1] for c in CC.TABLE]), np.array([c[2] for c in CC.TABLE], np.uint8)))
    for (name, _, _, want), row in zip(CC.TABLE, got):
        assert int(row[0]) | (int(row[1]) << 64) == CM.bits(want), name
    got = _u64(rules.threats(np.stack([CM.mirror(c[1]) for c in CC.TABLE]), np.array([1 - c[2] for c in CC.TABLE], np.uint8)))
    for (name, _, _, want), row in zip(CC.TABLE, got):
        assert int(row[0]) | (int(row[1]) << 64) == CM.bits([CM.mirror_sq(q) for q in want]), name


def test_random_playouts(rules):
    ref = CM.corpus_reference()
    assert len(ref[0]) >= 5000 and _hold(rules, ref) >= 0.25 * len(ref[0])


def test_golden_positions(rules, rules_golden):
    ref = CM.golden_reference(rules_golden)
    assert len(ref[0]) == 4381 and _hold(rules, ref) >= 400


@pytest.mark.parametrize("G", [1, 63, 64, 65, 4097, 400011])
def test_ragged_sizes_and_odd_addresses_raw_abi(rules, rules_golden, G):
    """Batch sizes around the wave's 64 positions; boards and side at a 16-byte aligned, an even and an odd byte address, the
    records at a 16-byte and at an 8-byte boundary; rows beyond the batch are not touched.  400 011 positions are 6 251 groups
    with a last one of 11, on a grid of 3 072 waves: every wave walks two or three groups, the next one prefetched."""
    from cchess_zero_amd._lib import check, lib
    boards, side, recs = CM.golden_reference(rules_golden)
    idx = (np.arange(G) * 37) % len(boards)
    for off, ooff in ((0, 0), (2, 8), (1, 0), (7, 8)):
        def buf(nbytes, o, fill):
            t = torch.full((nbytes + 32,), fill, dtype=torch.uint8, device="cuda")
            assert t.data_ptr() % 16 == 0
            return t[o:o + nbytes]
        b = buf(G * 90, off, 0)
        b.copy_(torch.from_numpy(np.ascontiguousarray(boards[idx]).reshape(-1)).cuda())
        s = buf(G, off, 0)
        s.copy_(torch.from_numpy(np.ascontiguousarray(side[idx])).cuda())
        out = buf((G + 2) * 32, ooff, 0x5A)
        rules.ctx.bind_stream()
        check(lib().cz_threats(rules.ctx.h, C.c_void_p(b.data_ptr()), C.c_void_p(s.data_ptr()), G, C.c_void_p(out.data_ptr())), "cz_threats")
        got = out.cpu().numpy().copy().view(np.uint64).reshape(G + 2, 4)
        assert np.array_equal(got[:G], recs[idx]), (off, ooff)
        assert (got[G:] == 0x5A5A5A5A5A5A5A5A).all()


def test_refused_boards_zero_batches_and_bad_arguments(rules, rules_golden):
    from cchess_zero_amd._lib import lib
    g = rules_golden
    bad = g["boards"][:4].copy()
    bad[2, :] = 0
    bad[2, :3] = 3                                            # three red rooks: refused whichever side is to move
    for sd in (0, 1):
        got = _u64(rules.threats(bad, np.full(4, sd, np.uint8)))
        assert (got[2] == 0).all() and (got[[0, 1, 3], 2:] != 0).any(axis=1).all()
    L, h = lib(), rules.ctx.h
    b, s = torch.from_numpy(bad).cuda(), torch.zeros(4, dtype=torch.uint8, device="cuda")
    out = torch.full((5, 4), 7, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.cz_threats(h, p(b), p(s), 0, p(out)) == 0 and L.cz_threats(h, None, None, 0, None) == 0     # G = 0: nothing happens
    assert (out.cpu().numpy() == 7).all()
    assert L.cz_threats(h, p(b), p(s), 4, None) == -1 and L.cz_threats(h, None, p(s), 4, p(out)) == -1
    assert L.cz_threats(None, p(b), p(s), 4, p(out)) == -1 and L.cz_threats(h, p(b), p(s), -1, p(out)) == -1
    assert L.cz_threats(h, p(b), p(s), 4, C.c_void_p(out.data_ptr() + 4)) == -1                            # not 8-byte aligned


@pytest.mark.parametrize("mirrored", [False, True])
def test_constructed_chase_ply_by_ply(rules, mirrored):
    """hash, in_check, threats and the verdict, all from the library: no verdict up to ply 7, the chaser loses at ply 8."""
    boards, sides, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE, mirrored)
    n = len(boards)
    keys = rules.hash(boards, sides)
    chk = rules.in_check(boards, sides) & 1
    recs = rules.threats(boards, sides)
    assert np.array_equal(_u64(recs), CM.records(boards, sides)) and not chk.any()
    length = np.arange(1, n + 1, dtype=np.int32)
    verdict, first, cause = rules.repetition_chase(keys.repeat(n, 1), chk.repeat(n, 1), recs.repeat(n, 1, 1), sides, length, None, 3)
    loser = CM.BLACK_LOSES if mirrored else CM.RED_LOSES
    assert verdict.cpu().numpy().tolist() == [0] * 8 + [loser]
    assert first.cpu().numpy().tolist() == [-1] * 8 + [0] and cause.cpu().numpy().tolist() == [0] * 8 + [CM.CAUSE_CHASE]
    plain, _ = rules.repetition(keys.repeat(n, 1), chk.repeat(n, 1), sides, length, None, 3)
    assert plain.cpu().numpy().tolist() == [0] * 8 + [CM.DRAW]


STRIDES = (9, 64, 65, 200)
WINDOWS = ("null", "zero", "all", "random")


@pytest.fixture(scope="module")
def launches():
    """One entry per launch: every (stride, fold, window kind), 45 games each = 2 160 records.  Keys from a small alphabet so
    that positions repeat, random check bits (a third of the games without any, a sixth with one side checking all the time),
    chase records of `stride` consecutive positions of the playout corpus (a sixth of the games with 65 and 200 positions:
    constructed far-reaching chases instead), with the model's answers."""
    _, cside, crecs = CM.corpus_reference()
    rng = np.random.default_rng(77)
    out = []
    for stride, fold, wk in itertools.product(STRIDES, (2, 3, 4), WINDOWS):
        G = 45
        keys = rng.integers(0, rng.choice([3, 5, 8], (G, 1)), (G, stride)).astype(np.uint64) ^ rng.integers(0, 1 << 63, (G, 1)).astype(np.uint64)
        checks = (rng.random((G, stride)) < 0.25).astype(np.uint8)
        recs = np.zeros((G, stride, 4), np.uint64)
        length = rng.integers(1, stride + 1, G).astype(np.int32)
        length[: G // 3] = stride
        side = np.zeros(G, np.uint8)
        for g in range(G):
            start = int(rng.integers(0, len(crecs) - stride))
            recs[g] = crecs[start:start + stride]
            side[g] = cside[start + length[g] - 1]
            kind = g % 6
            if kind < 2:
                checks[g] = 0
            elif kind == 2:
                checks[g, int(rng.integers(2))::2] = 1
            elif kind == 5 and stride >= 65:
                # a far-reaching cycle: the only repetitions are fold - 1 planted ones in the first third of the game, no checks,
                # and one side's standing piece is threatened all the way (constructed records) — in a third of these games
                # with one position in between where it is not
                n = int(length[g]) - 1
                keys[g] = np.arange(stride, dtype=np.uint64) + np.uint64(1000 * g)
                if n // 3 >= fold - 1:
                    keys[g, rng.choice(n // 3, fold - 1, replace=False)] = keys[g, n]
                checks[g] = 0
                par = int(rng.integers(2))
                recs[g] = np.array(CC.synthetic_cycle(par == 0, par == 1, plies=stride - 1)[2], np.uint64)
                if rng.random() < 0.33:
                    recs[g, 2 * int(rng.integers(n // 3, max(n // 2, n // 3 + 1))) + par, 0] = 0
        window = {"null": None, "zero": np.zeros(G, np.int32), "all": length - 1,
                  "random": np.array([rng.integers(-2, n + 3) for n in length], np.int32)}[wk]
        want = [CM.verdict(keys[g, :length[g]].tolist(), checks[g, :length[g]].tolist(), recs[g, :length[g]], int(side[g]),
                           None if window is None else int(window[g]), fold) for g in range(G)]
        plain = [RM.verdict(keys[g, :length[g]].tolist(), checks[g, :length[g]].tolist(), int(side[g]),
                            None if window is None else int(window[g]), fold) for g in range(G)]
        out.append(dict(G=G, stride=stride, fold=fold, keys=keys, checks=checks, recs=recs, length=length, side=side, window=window,
                        verdict=np.array([w[0] for w in want], np.uint8), first=np.array([w[1] for w in want], np.int32),
                        cause=np.array([w[2] for w in want], np.uint8), plain=np.array([w[0] for w in plain], np.uint8)))
    return out


def test_the_model_answers_every_verdict_and_cause_often(launches):
    assert sum(c["G"] for c in launches) >= 2000
    v = np.concatenate([c["verdict"] for c in launches])
    cause = np.concatenate([c["cause"] for c in launches])
    plain = np.concatenate([c["plain"] for c in launches])
    span = np.concatenate([c["length"] - 1 - c["first"] for c in launches])
    print("verdicts", np.bincount(v, minlength=4), "causes", np.bincount(cause, minlength=3), "draws turned into a loss", int(((plain == RM.DRAW) & (v != RM.DRAW)).sum()))
    assert (np.bincount(v, minlength=4) >= 100).all()
    assert (np.bincount(cause, minlength=3) >= 100).all()
    for code in (CM.RED_LOSES, CM.BLACK_LOSES):
        assert ((v == code) & (cause == CM.CAUSE_CHASE)).sum() >= 40 and ((v == code) & (cause == CM.CAUSE_CHECK)).sum() >= 40
    assert ((cause == CM.CAUSE_CHASE) & (span > 64)).sum() >= 3          # a chase found across the kernel's 64-position chunks
    assert ((v == CM.DRAW) & (plain == RM.DRAW)).sum() >= 100


def test_cz_repetition_chase_equals_the_model_and_cz_repetition_is_unchanged(rules, launches):
    for c in launches:
        keys, recs = c["keys"].view(np.int64), c["recs"].view(np.int64)
        verdict, first, cause = rules.repetition_chase(keys, c["checks"], recs, c["side"], c["length"], c["window"], c["fold"])
        tag = (c["stride"], c["fold"], None if c["window"] is None else c["window"][:4])
        assert np.array_equal(verdict.cpu().numpy(), c["verdict"]), tag
        assert np.array_equal(first.cpu().numpy(), c["first"]), tag
        assert np.array_equal(cause.cpu().numpy(), c["cause"]), tag
        plain, pfirst = rules.repetition(keys, c["checks"], c["side"], c["length"], c["window"], c["fold"])
        assert np.array_equal(plain.cpu().numpy(), c["plain"]) and np.array_equal(pfirst.cpu().numpy(), c["first"]), tag


def test_repetition_chase_refusals(rules):
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd.engine import _ptr
    keys = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    checks = torch.zeros((2, 4), dtype=torch.uint8, device="cuda")
    recs = torch.zeros((2, 4, 4), dtype=torch.int64, device="cuda")
    side = torch.zeros(2, dtype=torch.uint8, device="cuda")
    length = torch.full((2,), 4, dtype=torch.int32, device="cuda")
    verdict = torch.zeros(2, dtype=torch.uint8, device="cuda")
    L, h = lib(), rules.ctx.h

    def call(keys_=keys, recs_=recs, stride=4, fold=3, G=2, verdict_=verdict, length_=length, h_=h):
        return L.cz_repetition_chase(h_, _ptr(keys_), _ptr(checks), _ptr(recs_), stride, _ptr(length_), None, _ptr(side), G, fold, _ptr(verdict_), None, None)
    assert call() == 0
    for kw in (dict(fold=1), dict(fold=9), dict(keys_=None), dict(recs_=None), dict(stride=0), dict(G=-1), dict(verdict_=None),
               dict(length_=None), dict(h_=None)):
        assert call(**kw) == -1, kw                      # CZ_EINVAL
        assert L.cz_last_error()
    assert call(G=0) == 0
    bad = torch.tensor([0, 5], dtype=torch.int32, device="cuda")          # a length outside the row: no verdict, nothing read
    v, f, c = rules.repetition_chase(keys, checks, recs, side, bad, None, 2)
    assert v.cpu().numpy().tolist() == [0, 0] and f.cpu().numpy().tolist() == [-1, -1] and c.cpu().numpy().tolist() == [0, 0]
