"""cz_records_expand (csrc/cz_records.hip; records.RecordExpander) against its host statement, selfplay.to_dense of
records.mirror_records: the 342 golden records and the constructed edge records of records_cases.py (counts 0, 1, 64, 65, 128;
visits with zeros, none at all, a saturated one; both movers; the self-mirror start position; a child on a fixed-point label),
in batches of 1, W - 1, W, W + 1 records (W = records per workgroup) and all at once, with no mirror flags, all 0, all 1 and
alternating ones, at temperatures 1.0 and 0.5.  Every output lies between 256 sentinel bytes that must survive the launch, and
is itself filled with the sentinel before it: an element the kernel did not write shows.

pi: both sides evaluate the same float64 expression, softmax(1 / T * log(visits)); a device log / exp that differs in its last
bits moves the float64 result by ~1e-15 relative, against a float32 half-ulp of 6e-8, so it can change the final rounding at the
most: the support must be the host's exactly and every value equal or adjacent in float32 to the host's rounded one."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import records_cases as RC

pytestmark = pytest.mark.gpu

SENTINEL, FENCE = 0xA5, 256
OUTPUTS = (("planes", 9 * 10 * 14), ("pi", 2086), ("z", 1))   # float32 elements per record


@pytest.fixture(scope="module")
def ex():
    from cchess_zero_amd.records import RecordExpander
    return RecordExpander()


@pytest.fixture(scope="module")
def pool():
    """all records, the constructed ones first so that the small batches are made of them"""
    rec = RC.all_records()
    return np.concatenate([rec[342:], rec[:342]])


_host = {}


def host(pool, key, idx, flags, temperature):
    """to_dense(mirror_records(...)) of the pool's records idx, computed once per case"""
    from cchess_zero_amd.records import mirror_records
    from cchess_zero_amd.selfplay import to_dense
    k = (key, temperature)
    if k not in _host:
        m = mirror_records(pool[idx], flags)
        _host[k] = (m,) + to_dense(m, temperature, exact=True)
    return _host[k]


def raw(ex, rec, n, flags, temperature, null=()):
    """cz_records_expand through the C ABI, every output between FENCE sentinel bytes -> (rc, {name: f32 array}); asserts the sentinels"""
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd._lib import _ptr
    ex.ctx.bind_stream()
    bufs, ptrs = {}, []
    for name, width in OUTPUTS:
        if name in null:
            ptrs.append(None)
            continue
        bufs[name] = torch.full((FENCE + 4 * width * n + FENCE,), SENTINEL, dtype=torch.uint8, device=ex.dev)
        assert bufs[name].data_ptr() % 16 == 0
        ptrs.append(C.c_void_p(bufs[name].data_ptr() + FENCE))
    rc = lib().cz_records_expand(ex.ctx.h, _ptr(rec), n, _ptr(flags), temperature, *ptrs)
    torch.cuda.synchronize()
    out = {}
    for name, width in OUTPUTS:
        if name in bufs:
            h = bufs[name].cpu().numpy()
            assert (h[:FENCE] == SENTINEL).all() and (h[FENCE + 4 * width * n:] == SENTINEL).all(), "%s: bytes outside the output were written" % name
            out[name] = h[FENCE:FENCE + 4 * width * n].view(np.float32).reshape(n, width)
    return rc, out


def _sizes():
    from cchess_zero_amd.records import RECORDS_PER_WORKGROUP as W
    return [1, W - 1, W, W + 1, None]


@pytest.mark.parametrize("size", range(5))
def test_expansion_equals_the_host_statement(ex, pool, size):
    from cchess_zero_amd.rules import Rules
    n = _sizes()[size] or len(pool)
    # the small batches walk through the constructed records from the back: counts 128, 128, 65, 64, 1
    idx = np.arange(n) if n == len(pool) else (39 - 7 * np.arange(n)) % 40
    rules = Rules(ctx=ex.ctx)
    drec = torch.from_numpy(pool[idx]).to(ex.dev)
    kinds = {"null": None, "zeros": np.zeros(n, np.uint8), "ones": np.ones(n, np.uint8), "alternating": (np.arange(n) % 2 == 0).astype(np.uint8)}
    for kind, flags in kinds.items():
        dflags = None if flags is None else torch.from_numpy(flags).to(ex.dev)
        for temperature in (1.0, 0.5):
            m, planes, pi, z = host(pool, (size, kind), idx, np.zeros(n, np.uint8) if flags is None else flags, temperature)
            rc, out = raw(ex, drec, n, dflags, temperature)
            assert rc == 0, (kind, temperature)
            assert np.array_equal(out["planes"].reshape(n, 9, 10, 14), planes), (kind, temperature)
            assert np.array_equal(out["z"][:, 0], z), (kind, temperature)
            want = pi.astype(np.float32)
            got = out["pi"]
            assert np.array_equal(got != 0, want != 0), (kind, temperature)           # the support, exactly
            ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            print("n %d flags %s T %.1f: pi differs from the host's float32 in %d of %d non-zero cells, by at most %d ulp"
                  % (n, kind, temperature, int((ulps > 0).sum()), int((want != 0).sum()), int(ulps.max())))
            assert ulps.max() <= 1, (kind, temperature, int(ulps.max()))                # equal or adjacent in float32
        # ... and the planes are the encoder's of the mirrored boards
        enc = rules.encode_planes(m[:, :90], m[:, 90])
        assert np.array_equal(enc.cpu().numpy(), planes), kind


def test_mirror_flag_is_the_expansion_of_the_mirrored_record(ex, pool):
    """the same arithmetic on permuted inputs: bit for bit on all three outputs"""
    from cchess_zero_amd.records import mirror_records
    n = len(pool)
    for temperature in (1.0, 0.5):
        a = ex.expand(pool, mirror=np.ones(n, np.uint8), temperature=temperature)
        b = ex.expand(mirror_records(pool), mirror=np.zeros(n, np.uint8), temperature=temperature)
        c = ex.expand(torch.from_numpy(mirror_records(pool)).to(ex.dev), temperature=temperature)   # a device tensor, no flags
        for x, y, w in zip(a, b, c):
            assert x.dtype == torch.float32 and x.device == ex.dev and torch.equal(x, y) and torch.equal(x, w)
    assert a[0].shape == (n, 9, 10, 14) and a[1].shape == (n, 2086) and a[2].shape == (n,)


def test_arguments_through_the_c_abi(ex, pool):
    from cchess_zero_amd._lib import lib
    drec = torch.from_numpy(pool[:8]).to(ex.dev)
    rc, out = raw(ex, drec, 0, None, 1.0)           # n = 0: nothing launched, nothing written (raw() asserts the sentinels)
    assert rc == 0 and all(v.size == 0 for v in out.values())
    for kwargs in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=1.0, null=("planes",)), dict(temperature=1.0, null=("pi",)),
                   dict(temperature=1.0, null=("z",))):
        rc, out = raw(ex, drec, 8, None, **kwargs)
        assert rc != 0 and b"cz_records_expand" in lib().cz_last_error(), kwargs
        for v in out.values():                       # a refused call writes nothing
            assert (v.view(np.uint8) == SENTINEL).all()
    assert lib().cz_records_expand(ex.ctx.h, None, -1, None, 1.0, None, None, None) != 0 and b"cz_records_expand" in lib().cz_last_error()


def test_policy_update_with_the_expander(ex, pool, tmp_path):
    from policy_value_network import policy_value_network
    from cchess_zero_amd.train import policy_update
    net = policy_value_network(1, save_dir=str(tmp_path), seed=3)
    buf = [r for r in pool]
    seed = 5
    rng = random.Random((seed << 32) ^ int(net.global_step))
    rng.sample(range(len(buf)), 8)
    coins = sum(rng.getrandbits(1) for _ in range(8))
    _, info = policy_update(net, buf, 8, 1, 0.02, 1.0, 0.025, seed=seed, log=lambda *a: None, mirror=True, expand=ex.expand)
    assert info["steps"] == 1 and np.isfinite(float(info["loss"]))
    assert info["mirrored"] == coins
