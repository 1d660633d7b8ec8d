"""cz_mate_backup on the GPU against tests/mate_model.backup, bit for bit, through the raw C ABI with sentinel bytes behind both
outputs: parents around the block's and the wave's sizes, child counts 0 .. 128, lines of 0, 1 and 14 moves, both modes, ties
at the minimum and the maximum, parents whose children are all unproven or hold one unproven child, and offsets that run past
the children."""
import ctypes as C

import numpy as np
import pytest
import torch

import mate_model as MM

pytestmark = pytest.mark.gpu
NONE = MM.NONE
COUNTS = (0, 1, 2, 63, 64, 65, 128)


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


def _case(G, W, seed):
    """Parents with child counts from COUNTS (every one of them occurs when G allows); distances from a small range, so that
    ties are the rule; parent g % 4 == 1 has only unproven children, g % 4 == 2 exactly one unproven child among proven ones."""
    rng = np.random.default_rng(seed)
    counts = np.array([COUNTS[(g + seed) % len(COUNTS)] for g in range(G)], np.int64)
    offsets = np.zeros(G + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    T = int(offsets[-1])
    dist = rng.integers(0, 4, T).astype(np.int16) * 2                # 0, 2, 4, 6: many ties at either end
    for g in range(G):
        lo, hi = offsets[g], offsets[g + 1]
        if g % 4 == 1:
            dist[lo:hi] = NONE
        elif g % 4 == 2 and hi > lo:
            dist[lo + int(rng.integers(0, hi - lo))] = NONE
    label = rng.integers(0, 2086, T).astype(np.uint16)
    pv = rng.integers(0, 2086, (T, W)).astype(np.uint16)
    pv[rng.random((T, W)) < 0.2] = 0xFFFF
    return offsets, T, dist, label, pv


def _raw(rules, offsets, T, dist, label, pv, W, mode, G=None, total=None, sentinel=0x5A):
    from cchess_zero_amd._lib import check, lib
    G = len(offsets) - 1 if G is None else G
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a.size else None
    d_off, d_dist, d_label, d_pv = dev(offsets), dev(dist.view(np.int16)), dev(label.view(np.int16)), dev(pv.view(np.int16)) if W else None
    od = torch.full(((G + 2) * 2,), sentinel, dtype=torch.uint8, device="cuda")
    op = torch.full(((G + 2) * 2 * (W + 1),), sentinel, dtype=torch.uint8, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rules.ctx.bind_stream()
    check(lib().cz_mate_backup(rules.ctx.h, p(d_off), G, T if total is None else total, p(d_dist), p(d_label), p(d_pv), W, mode, p(od), p(op)), "cz_mate_backup")
    return od.cpu().numpy().view(np.int16), op.cpu().numpy().view(np.uint16).reshape(G + 2, W + 1)


@pytest.mark.parametrize("W", [0, 1, 14])
@pytest.mark.parametrize("G", [1, 63, 64, 65, 129])
def test_both_modes_against_the_model(rules, G, W):
    for mode in (0, 1):
        for seed in range(len(COUNTS) if G == 1 else 2):              # a single parent takes every child count in turn
            offsets, T, dist, label, pv = _case(G, W, seed)
            want_d, want_pv = MM.backup(offsets, T, dist, label, pv, W, mode)
            got_d, got_pv = _raw(rules, offsets, T, dist, label, pv, W, mode)
            assert np.array_equal(got_d[:G], want_d), (mode, seed, np.nonzero(got_d[:G] != want_d)[0][:5])
            assert np.array_equal(got_pv[:G], want_pv), (mode, seed, np.nonzero((got_pv[:G] != want_pv).any(axis=1))[0][:5])
            assert (got_d[G:] == 0x5A5A).all() and (got_pv[G:] == 0x5A5A).all()


def test_the_cases_hold_what_they_promise():
    """Ties, all-unproven parents, one unproven child among proven ones, childless parents: present in the generated cases, and
    the model answers them as the contract says."""
    offsets, T, dist, label, pv = _case(129, 1, 0)
    d0, p0 = MM.backup(offsets, T, dist, label, pv, 1, 0)
    d1, p1 = MM.backup(offsets, T, dist, label, pv, 1, 1)
    n = np.diff(offsets)
    ties = all_none = one_none = 0
    for g in range(129):
        c = dist[offsets[g]:offsets[g + 1]].astype(np.int64)
        proven = c[c != NONE]
        if n[g] == 0:
            assert d0[g] == NONE and d1[g] == 0 and (p0[g] == 0xFFFF).all() and (p1[g] == 0xFFFF).all()
        elif len(proven) == 0:
            all_none += 1
            assert d0[g] == NONE and d1[g] == NONE and (p0[g] == 0xFFFF).all()
        elif len(proven) < n[g]:
            one_none += 1
            first = int(np.nonzero(c == proven.min())[0][0])
            assert d0[g] == proven.min() + 1 and d1[g] == NONE and p0[g, 0] == label[offsets[g] + first] and (p1[g] == 0xFFFF).all()
        else:
            ties += int((c == c.min()).sum() > 1 and (c == c.max()).sum() > 1)
            assert d0[g] == c.min() + 1 and d1[g] == c.max() + 1
            assert p0[g, 0] == label[offsets[g] + int(np.argmin(c))] and p1[g, 0] == label[offsets[g] + int(np.argmax(c))]
    assert (n == 0).sum() >= 10 and all_none >= 20 and one_none >= 20 and ties >= 10


def test_offsets_that_run_past_the_children_are_clamped(rules):
    """Negative offsets, offsets beyond `total`, a decreasing pair, and a `total` smaller than the arrays: the kernel reads the
    clamped ranges (the model clamps alike) and writes nothing outside its G rows."""
    G, W = 70, 3
    offsets, T, dist, label, pv = _case(G, W, 1)
    wild = offsets.copy()
    wild[3], wild[10], wild[20], wild[40], wild[G] = -5, T + 1000, wild[19] - 7, 2 ** 31 - 1, T + 5
    for mode in (0, 1):
        for total in (T, T // 2):
            want_d, want_pv = MM.backup(wild, total, dist, label, pv, W, mode)
            got_d, got_pv = _raw(rules, wild, T, dist, label, pv, W, mode, total=total)
            assert np.array_equal(got_d[:G], want_d) and np.array_equal(got_pv[:G], want_pv), (mode, total)
            assert (got_d[G:] == 0x5A5A).all() and (got_pv[G:] == 0x5A5A).all()


def test_rules_wrapper_and_argument_errors(rules):
    from cchess_zero_amd._lib import CchessHipError
    offsets, T, dist, label, pv = _case(65, 2, 0)
    for mode in (0, 1):
        d, line = rules.mate_backup(offsets, dist, label.view(np.int16), pv.view(np.int16), mode)
        want_d, want_pv = MM.backup(offsets, T, dist, label, pv, 2, mode)
        assert np.array_equal(d.cpu().numpy(), want_d) and np.array_equal(line.cpu().numpy().view(np.uint16), want_pv)
    d, line = rules.mate_backup(np.zeros(4, np.int32), np.zeros(0, np.int16), np.zeros(0, np.int16), None, 1)      # three childless defenders
    assert d.cpu().numpy().tolist() == [0, 0, 0] and (line.cpu().numpy() == -1).all() and line.shape == (3, 1)
    with pytest.raises(CchessHipError, match="mode"):
        _raw(rules, offsets, T, dist, label, pv, 2, 2)
    with pytest.raises(CchessHipError, match="W is"):
        _raw(rules, offsets, T, dist, label, pv, -1, 0)
    with pytest.raises(CchessHipError, match="negative"):
        _raw(rules, offsets, T, dist, label, pv, 2, 0, G=-1)
