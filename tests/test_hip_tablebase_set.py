"""The one-launch mixed probe on the GPU (cz_tb_set_create / cz_tb_set_probe, k_tb_probe_set; Tablebase.device_set / probe_set)
held to Tablebase.probe — which groups the boards on the host and launches one cz_tb_probe per signature — bit for bit, and to
tests/tablebase_set_model.py on the recorded tables.  The tables are built once per module, as tests/test_hip_tablebase.py's."""
import ctypes as C

import numpy as np
import pytest

import tablebase_model as TM
import tablebase_set_model as SM

pytestmark = pytest.mark.gpu

ILLEGAL, MISS = TM.ILLEGAL, TM.MISS
BUILD = ("KP-KP", "KR-KAA", "KN-KA", "KN-KB", "KR-K", "KC-K")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tb():
    from cchess_zero_amd.tablebase import Tablebase
    t = Tablebase()
    for s in BUILD:
        t.build(s)
    return t


def _special_boards():
    """(name, board, side): the boards no table index gives"""
    from cchess_zero_amd.rules import START_BOARD
    start = np.asarray(START_BOARD, np.uint8).reshape(90)
    out = [("start", start, 0)]
    no_king = np.zeros(90, np.uint8)
    no_king[[4, 40]] = (1, 3)
    out.append(("no black king", no_king, 0))
    krr = np.zeros(90, np.uint8)
    krr[[4, 36, 37, 85]] = (1, 3, 3, 8)
    out.append(("KRR-K is in no set", krr, 1))
    a = np.zeros(90, np.uint8)
    a[[3, 10, 85, 66, 68]] = (1, 3, 8, 9, 9)   # the kings on different files
    out.append(("KR-KAA", a, 0))
    swapped = a.copy()                   # the same two advisors: among equal pieces the order of the squares is the slots'
    out.append(("KR-KAA again", swapped, 1))
    wide = a.copy()
    wide[[66, 68]] = 0
    wide[[84, 86]] = 9
    out.append(("KR-KAA, the advisors on other squares", wide, 0))
    outside = a.copy()
    outside[68], outside[67] = 0, 9
    out.append(("an advisor outside its domain", outside, 0))
    king_out = a.copy()
    king_out[3], king_out[40] = 0, 1
    out.append(("a king outside the palace", king_out, 1))
    for byte in (15, 16, 0x11, 200):
        f = a.copy()
        f[30] = byte
        out.append(("byte %d" % byte, f, 0))
    eleven = start.copy()
    eleven[np.nonzero(start)[0][11:]] = 0
    assert int((eleven != 0).sum()) == 11
    out.append(("11 pieces", eleven, 0))
    twelve = start.copy()
    twelve[np.nonzero(start)[0][:20]] = 0
    assert int((twelve != 0).sum()) == 12
    out.append(("12 pieces", twelve, 1))
    ten = np.zeros(90, np.uint8)         # ten pieces of a signature nobody built
    ten[[4, 85, 0, 8, 1, 7, 81, 89, 82, 88]] = (1, 8, 3, 3, 5, 5, 10, 10, 12, 12)
    out.append(("KRRNN-KRRNN", ten, 0))
    return out


@pytest.fixture(scope="module")
def batch(tb, torch):
    """A shuffled mixed batch: boards of every loaded table (overlapping indices included: empty boards) and the special ones
    -> boards, side (device), the signature index of every board (-1: special), the reference's answer"""
    g = torch.Generator().manual_seed(3)
    sigs = sorted(tb.tables)
    boards, side, owner = [], [], []
    for k, s in enumerate(sigs):
        n = tb.tables[s].numel()
        idx = torch.randint(0, n, (200,), generator=g).to(torch.int32)
        b, sd = tb.boards(s, idx)
        boards.append(b)
        side.append(sd)
        owner += [k] * 200
    sp = _special_boards()
    boards.append(torch.from_numpy(np.stack([b for _, b, _ in sp])).to(tb.dev))
    side.append(torch.tensor([s for _, _, s in sp], dtype=torch.uint8, device=tb.dev))
    owner += [-1] * len(sp)
    boards, side, owner = torch.cat(boards), torch.cat(side), torch.tensor(owner)
    perm = torch.randperm(boards.shape[0], generator=g)
    boards, side, owner = boards[perm.to(tb.dev)].contiguous(), side[perm.to(tb.dev)].contiguous(), owner[perm]
    value, covered = tb.probe(boards, side)          # the reference, computed once
    return dict(boards=boards, side=side, owner=owner, sigs=sigs, value=value, covered=covered, names=[n for n, _, _ in sp], perm=perm)


def _which_reference(tb, batch):
    """the place of every board's signature in sorted(tb.tables), -1 for a miss: from Tablebase.signatures_of"""
    sigs, group = tb.signatures_of(batch["boards"])
    place = [batch["sigs"].index(s) if s in tb.tables else -1 for s in sigs]
    return np.array(place, np.int32)[group.cpu().numpy()]


def test_a_mixed_batch_equals_probe_bit_for_bit(tb, torch, batch):
    G = batch["boards"].shape[0]
    assert G > 2000 and len(batch["sigs"]) >= 14
    # not vacuous: single waves hold at least three signatures, and every kind of answer occurs
    own = batch["owner"].numpy()
    assert min(len(set(own[i:i + 64].tolist()) - {-1}) for i in range(0, G - 63, 64)) >= 3
    ref = batch["value"].cpu().numpy()
    assert (ref == MISS).any() and (ref == ILLEGAL).any() and (ref == 0).any() and ((ref > 0) & (ref < MISS)).any() and ((ref < 0) & (ref > ILLEGAL)).any()
    value, covered, which = tb.probe_set(batch["boards"], batch["side"])
    assert value.dtype == torch.int16 and which.dtype == torch.int32
    bad = np.nonzero(value.cpu().numpy() != ref)[0]
    assert len(bad) == 0, (len(bad), bad[:5], value.cpu().numpy()[bad[:5]], ref[bad[:5]])
    assert torch.equal(covered, batch["covered"])
    assert np.array_equal(which.cpu().numpy(), _which_reference(tb, batch))
    # the special boards, by name: what each must answer
    at = {n: int(np.nonzero(batch["perm"].numpy() == G - len(batch["names"]) + i)[0][0]) for i, n in enumerate(batch["names"])}
    v = value.cpu().numpy()
    for n in ("start", "no black king", "KRR-K is in no set", "byte 15", "byte 16", "byte 17", "byte 200", "11 pieces", "12 pieces", "KRRNN-KRRNN"):
        assert v[at[n]] == MISS and int(which[at[n]]) == -1, n
    for n in ("an advisor outside its domain", "a king outside the palace"):
        assert v[at[n]] == ILLEGAL and int(which[at[n]]) == batch["sigs"].index("KR-KAA"), n
    for n in ("KR-KAA", "KR-KAA again", "KR-KAA, the advisors on other squares"):
        assert v[at[n]] not in (MISS, ILLEGAL), n


@pytest.mark.parametrize("G", [1, 63, 64, 65])
def test_group_sizes(tb, torch, batch, G):
    value, covered, which = tb.probe_set(batch["boards"][:G].contiguous(), batch["side"][:G].contiguous())
    assert torch.equal(value, batch["value"][:G]) and torch.equal(covered, batch["covered"][:G])
    assert np.array_equal(which.cpu().numpy(), _which_reference(tb, batch)[:G])


def test_empty_unaligned_and_no_which(tb, torch, batch):
    from cchess_zero_amd._lib import call
    dset = tb.device_set()
    try:
        tb.ctx.bind_stream()
        assert call("cz_tb_set_probe", tb.ctx.h, dset.h, None, None, 0, None, None) == 0            # G == 0: no launch, nothing is read
        G = 300
        raw = torch.zeros(G * 90 + 16, dtype=torch.uint8, device=tb.dev)
        for off in (2, 7):                                                                           # not 16-byte aligned
            view = raw[off:off + G * 90]
            view.copy_(batch["boards"][:G].reshape(-1))
            assert view.data_ptr() % 16 != 0
            value = torch.full((G + 1,), 12345, dtype=torch.int16, device=tb.dev)
            tb.ctx.call("cz_tb_set_probe", dset.h, view, batch["side"][:G].contiguous(), G, value, None)   # which = NULL
            assert torch.equal(value[:G], batch["value"][:G]) and int(value[G]) == 12345
    finally:
        dset.close()


def test_one_signature_and_reverse_order(tb, torch, batch):
    sigs = batch["sigs"]
    ref_which = _which_reference(tb, batch)
    one = tb.device_set(["KR-KAA"])
    rev = tb.device_set(list(reversed(sigs)))
    try:
        value, covered, which = tb.probe_set(batch["boards"], batch["side"], one)
        mine = torch.from_numpy(ref_which == sigs.index("KR-KAA")).to(tb.dev)
        assert bool(mine.any()) and torch.equal(value[mine], batch["value"][mine]) and bool((value[~mine] == MISS).all())
        assert bool((which[mine] == 0).all()) and bool((which[~mine] == -1).all())
        value, covered, which = tb.probe_set(batch["boards"], batch["side"], rev)
        assert torch.equal(value, batch["value"]) and torch.equal(covered, batch["covered"])
        want = np.where(ref_which >= 0, len(sigs) - 1 - ref_which, -1)
        assert np.array_equal(which.cpu().numpy(), want)
    finally:
        one.close()
        rev.close()


def test_against_the_model_on_the_recorded_tables(tb, torch):
    values, _ = TM.golden()
    order = ["KN-KA", "K-K", "KP-K"]
    rng = np.random.default_rng(4)
    boards, side, want = [], [], []
    for s in order + ["KR-K"]:            # KR-K is loaded but not in this set: a miss
        for i in rng.integers(TM.entries(s), size=150):
            b, sd = TM.unrank(s, int(i))
            b = np.zeros(90, np.uint8) if b is None else b
            boards.append(b)
            side.append(sd)
            want.append(SM.probe(values, order, b, sd))
    for s in order:
        assert np.array_equal(tb.tables[s].cpu().numpy(), values[s])
    dset = tb.device_set(order)
    try:
        value, covered, which = tb.probe_set(np.stack(boards), np.array(side, np.uint8), dset)
    finally:
        dset.close()
    assert value.cpu().tolist() == [v for v, _ in want] and which.cpu().tolist() == [w for _, w in want]
    assert covered.cpu().tolist() == [SM.covered(v) for v, _ in want]
    assert len({w for _, w in want}) == 4 and any(v == ILLEGAL for v, _ in want)


def test_a_wave_of_one_entry_and_a_wave_of_misses(tb, torch):
    """Groups of 64 that hold one signature only (the waterfall runs once) and none at all (it never runs), beside a mixed one"""
    from cchess_zero_amd.rules import START_BOARD
    n = tb.tables["KR-KAA"].numel()
    idx = (torch.arange(64, dtype=torch.int64) * 5651 % n).to(torch.int32)
    same, same_side = tb.boards("KR-KAA", idx)
    keep = (same != 0).any(1)
    same[~keep] = same[keep][0]           # no empty board among the 64: every lane holds the one entry
    same_side[~keep] = same_side[keep][0]
    miss = torch.from_numpy(np.tile(np.asarray(START_BOARD, np.uint8).reshape(1, 90), (64, 1))).to(tb.dev)
    mixed, mixed_side = tb.boards("KN-KB", torch.arange(0, 6400, 100, dtype=torch.int32))
    boards = torch.cat([same, miss, mixed, miss[:5]]).contiguous()
    side = torch.cat([same_side, torch.zeros(64, dtype=torch.uint8, device=tb.dev), mixed_side, torch.ones(5, dtype=torch.uint8, device=tb.dev)]).contiguous()
    ref, ref_cov = tb.probe(boards, side)
    value, covered, which = tb.probe_set(boards, side)
    assert torch.equal(value, ref) and torch.equal(covered, ref_cov)
    sigs = sorted(tb.tables)
    assert which[:64].cpu().tolist() == [sigs.index("KR-KAA")] * 64 and bool((value[:64] != MISS).all())
    assert which[64:128].cpu().tolist() == [-1] * 64 and bool((value[64:128] == MISS).all()) and which[-5:].cpu().tolist() == [-1] * 5


def test_refusals_and_their_texts(tb, torch):
    from cchess_zero_amd._lib import CchessHipError, lib
    L = lib()
    ptr = tb.tables["KR-K"].data_ptr()

    def create(sigs, ptrs):
        names = (C.c_char_p * max(len(sigs), 1))(*[s if s is None else s.encode() for s in sigs])
        arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        h = C.c_void_p()
        rc = L.cz_tb_set_create(tb.ctx.h, len(sigs), names, arr, C.byref(h))
        return rc, (L.cz_last_error() or b"").decode(), h
    for sigs, ptrs, text in (([], [], "1 <= n <= 256"),
                             (["KR-K", "KR+K"], [ptr, ptr], 'cz_tb_set_create: bad signature "KR+K": red pieces, \'-\', black pieces, of the letters KRNCPAB'),
                             (["KAR-K"], [ptr], 'bad signature "KAR-K": letters in the order KRNCPAB'),
                             (["KR-K", "KN-K", "KR-K"], [ptr, ptr, ptr], 'signature "KR-K" given twice'),
                             (["KR-K"], [None], 'tables[0] (the table of "KR-K") required, 2-byte aligned'),
                             (["KN-K", "KR-K"], [ptr, ptr + 1], 'tables[1] (the table of "KR-K") required, 2-byte aligned')):
        rc, msg, h = create(sigs, ptrs)
        assert rc == -1 and text in msg and not h.value, (sigs, rc, msg)
    rc, msg, h = create(["KR-K"] * 257, [ptr] * 257)
    assert rc == -1 and "1 <= n <= 256" in msg
    with pytest.raises(KeyError):
        tb.device_set(["KR-K", "KRR-K"])            # not loaded
    dset = tb.device_set(["KR-K"])
    try:
        b, s = tb.boards("KR-K", [0, 1])
        v = torch.empty(3, dtype=torch.int16, device=tb.dev)
        for args, text in (((None, b, s, 2, v, None), "null set"), ((dset.h, None, s, 2, v, None), "boards, side, value required"),
                           ((dset.h, b, s, -1, v, None), "negative G"), ((dset.h, b, s, 2, C.c_void_p(v.data_ptr() + 1), None), "value must be 2-byte"),
                           ((dset.h, b, s, 2, v, C.c_void_p(v.data_ptr() + 2)), "which 4-byte aligned")):
            with pytest.raises(CchessHipError, match=text):
                tb.ctx.call("cz_tb_set_probe", *args)
    finally:
        dset.close()
    assert dset.h is None
