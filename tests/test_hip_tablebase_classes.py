"""The tablebase kernels (cz_tb_pass, cz_tb_probe, cz_tb_boards) on the material classes tests/test_hip_tablebase.py does not reach,
none of which tests/tablebase_model.py can build in reasonable time: the red advisor and elephant domains, tables that black
wins, two equal pieces on the 55- and 90-square domains, six and seven slots (cz_tb_boards: ten), indices above 2^24.
  1. KR-KAB, KAB-KR, KPP-K, K-KPP: passes, counts, longest lines and crc32 of the HOST build of cz_tablebase.h
     (tests/tablebase_classes.py PINNED, which tests/test_tablebase_classes_cpu.py re-measures);
  2. flip, mirror and canonical identities over every index of eight tables up to 1 559 250 entries;
  3. KR-KAABB (17 860 500 entries, 7 slots) on a sample of every 61st index: the pass rule on the children's final values, mirror,
     canonical, the ILLEGAL entries;
  4. the pass rule over every legal index of KP-KAAB and KNN-K;
  5. Rules.mate against KAB-KR, which black wins;
  6. Tablebase.best on wins, losses and draws of KR-KAB;
  7. cz_tb_boards on the ten slots of KAABB-KAABB against the model's unrank.
Every comparison is equality.  One Tablebase builds everything once per module."""
import time

import numpy as np
import pytest

import tablebase_classes as TC
import tablebase_model as TM

pytestmark = pytest.mark.gpu

ILLEGAL = TM.ILLEGAL
PAIRS = (("KR-KAB", "KAB-KR"), ("KPP-K", "K-KPP"), ("KNN-K", "K-KNN"), ("KP-KAAB", "KAAB-KP"))
BIG = "KR-KAABB"


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tb(torch):
    from cchess_zero_amd.tablebase import Tablebase
    t = Tablebase()
    start = time.perf_counter()
    for a, b in PAIRS:
        t.build(a)
        t.build(b)
    torch.cuda.synchronize()
    pairs = time.perf_counter() - start
    t.build(BIG)
    torch.cuda.synchronize()
    print("built %d tables: the four pairs and their closures in %.2f s, %s and its closure in %.2f s"
          % (len(t.tables), pairs, BIG, time.perf_counter() - start - pairs))
    return t


@pytest.fixture(scope="module")
def src(tb):
    return TC.DeviceTables(tb)


@pytest.fixture(scope="module")
def big_sample(tb, torch):
    """indices 0 .. 127, the last 128 and every 61st (61 is coprime to 2 and to every radix: both sides and all digits vary)"""
    n = tb.tables[BIG].numel()
    assert n == 17860500
    dev = tb.tables[BIG].device
    idx = torch.unique(torch.cat([torch.arange(128, device=dev), torch.arange(n - 128, n, device=dev), torch.arange(0, n, 61, device=dev)]))
    v = tb.tables[BIG][idx].to(torch.int32)
    return idx, v


@pytest.mark.parametrize("sig", sorted(TC.PINNED))
def test_bit_for_bit_against_the_host_build(tb, sig):
    got = TC.table_stats(tb.tables[sig], tb.stats[sig]["passes"])
    print("%s: %s" % (sig, {k: ("%08x" % v if k == "crc32" else v) for k, v in got.items()}))
    assert got == TC.PINNED[sig]
    assert {k: tb.stats[sig][k] for k in ("entries", "legal", "wins", "losses", "longest_win", "longest_loss")} == {k: got[k] for k in got if k not in ("passes", "crc32")}


@pytest.mark.parametrize("a,b", PAIRS)
def test_flip(tb, src, a, b):
    seen = TC.check_flip(src, a, b)
    assert seen["legal"] == tb.stats[a]["legal"] > 0
    for k in ("entries", "legal", "wins", "losses", "draws", "longest_win", "longest_loss", "passes"):
        assert tb.stats[a][k] == tb.stats[b][k], (k, tb.stats[a], tb.stats[b])
    assert tb.stats[a]["wins"] > 0 and tb.stats[a]["losses"] > 0


@pytest.mark.parametrize("sig", [s for p in PAIRS for s in p])
def test_mirror(tb, src, sig):
    assert TC.check_mirror(src, sig)["legal"] == tb.stats[sig]["legal"]


@pytest.mark.parametrize("sig", ["KPP-K", "K-KPP", "KNN-K", "K-KNN", "KP-KAAB"])
def test_canonical(src, sig):
    other = TC.check_canonical(src, sig)
    assert other == TC.NON_CANONICAL.get(sig, other)


def test_seven_slots_sampled(tb, src, torch, big_sample):
    idx, v = big_sample
    legal = idx[v != ILLEGAL]
    lv = v[v != ILLEGAL]
    print("%s: %d sampled, %d legal, %d wins, %d losses, %d draws, %d above 2^24, passes %d" % (
        BIG, idx.numel(), legal.numel(), int((lv > 0).sum()), int((lv < 0).sum()), int((lv == 0).sum()), int((idx > 1 << 24).sum()), tb.stats[BIG]["passes"]))
    assert legal.numel() >= 100000 and bool((lv > 0).any()) and bool((lv < 0).any()) and bool((legal > 1 << 24).any())
    TC.check_fixpoint(tb, BIG, legal)
    apart, overlapping = TC.check_illegal(tb, BIG, idx[v == ILLEGAL])
    assert apart > 0 and overlapping > 0


def test_seven_slots_sampled_symmetries(src, big_sample):
    idx, v = big_sample
    assert TC.check_mirror(src, BIG, idx)["legal"] == int((v != ILLEGAL).sum())
    assert TC.check_canonical(src, BIG, idx) > 0


@pytest.mark.parametrize("sig", ["KP-KAAB", "KNN-K"])
def test_fixpoint_over_every_index(tb, torch, sig):
    table = tb.tables[sig]
    legal = (table != ILLEGAL).nonzero().flatten()
    seen = TC.check_fixpoint(tb, sig, legal)
    assert seen["parents"] == tb.stats[sig]["legal"] and seen["batches"] > 1
    apart, overlapping = TC.check_illegal(tb, sig, (table == ILLEGAL).nonzero().flatten())
    assert apart > 0 and overlapping > 0


def test_against_the_mate_search_where_black_wins(tb, torch):
    """KAB-KR: Rules.mate over all king-safe moves proves exactly the table's wins within 5 plies, at their distance.  The search
    walks the whole tree (some 250 000 positions below a root with the rook to move), so the roots are a sample: every k-th of the
    near wins with black to move, of those with red to move (black stalemated into a loss), and of all other legal positions."""
    sig = "KAB-KR"
    v = tb.tables[sig].to(torch.int32)
    side = torch.arange(v.numel(), device=v.device) & 1
    legal = v != ILLEGAL
    near = legal & (v > 0) & (v - 1 <= 5)
    groups = [(near & (side == 1)).nonzero().flatten(), (near & (side == 0)).nonzero().flatten(), (legal & ~near).nonzero().flatten()]
    print("%s: %d wins within 5 plies with black to move, %d with red to move, %d other legal positions" % ((sig,) + tuple(int(g.numel()) for g in groups)))
    assert groups[0].numel() > 100
    roots = torch.cat([g[::max(1, g.numel() // k)][:k] for g, k in zip(groups, (1000, 200, 1000))])
    boards, rside = tb.boards(sig, roots.to(torch.int32))
    res = tb.rules.mate(boards, rside, 5, attacker="all")
    rv = v[roots].cpu().numpy()
    rnear = (rv > 0) & (rv - 1 <= 5)
    print("%d roots, %d near wins (%d with black to move), distances %s, %d positions made" % (
        roots.numel(), rnear.sum(), (rnear & (rside.cpu().numpy() == 1)).sum(), np.unique(rv[rnear] - 1).tolist(), int(res["nodes"].sum())))
    assert (rnear & (rside.cpu().numpy() == 1)).sum() > 100 and (~rnear).sum() > 100
    assert np.array_equal(res["status"][rnear], np.ones(rnear.sum(), np.uint8)), np.nonzero(res["status"][rnear] != 1)[0][:5]
    assert np.array_equal(res["dist"][rnear], (rv[rnear] - 1).astype(np.int16))
    assert not res["status"][~rnear].any(), (np.nonzero(res["status"][~rnear])[0][:5], np.unique(res["status"][~rnear]))


def test_best_on_every_class_of_value(tb, torch):
    """KR-KAB, 2 000 legal positions that have a move: the label is a move, the child is the position after it and holds the
    optimal value; on 50 of them the label is the FIRST such move of the model's king-safe list"""
    import kingsafe_model as M
    from perft_model import make_move
    sig = "KR-KAB"
    v = tb.tables[sig].to(torch.int32)
    have = ((v != ILLEGAL) & (v != -1)).nonzero().flatten()
    pick = have[::have.numel() // 2000][:2000]
    assert pick.numel() == 2000
    boards, side = tb.boards(sig, pick.to(torch.int32))
    pv = v[pick]
    print("%s: %d positions: %d wins, %d losses, %d draws" % (sig, pick.numel(), int((pv > 0).sum()), int((pv < 0).sum()), int((pv == 0).sum())))
    assert bool((pv > 0).any()) and bool((pv < 0).any()) and bool((pv == 0).any())
    label, value, nb, ns = tb.best(boards, side)
    assert torch.equal(value.to(torch.int32), pv) and bool((label >= 0).all())
    assert torch.equal(ns, 1 - side)
    want = torch.where(pv > 0, 1 - pv, torch.where(pv < 0, -pv - 1, torch.zeros_like(pv)))
    cv, covered = tb.probe(nb, ns)
    assert bool(covered.all()) and torch.equal(cv.to(torch.int32), want)
    hb, hs, hl, hn, hw = boards.cpu().numpy(), side.cpu().numpy(), label.cpu().numpy(), nb.cpu().numpy(), want.cpu().numpy()
    for k in range(2000):
        assert np.array_equal(hn[k], make_move(hb[k], int(hl[k]))[0]), k
    # the first optimal move in the model's list order: three of each class of value at least, 50 in all
    hv = pv.cpu().numpy()
    some = sorted(set(np.nonzero(hv > 0)[0][:3].tolist() + np.nonzero(hv < 0)[0][:3].tolist() + np.nonzero(hv == 0)[0][:3].tolist() + list(range(0, 2000, 40))))[:50]
    assert len(some) == 50
    lists = [[int(m) for m in M.kingsafe(hb[k], int(hs[k]))[0]] for k in some]
    kids = np.stack([make_move(hb[k], m)[0] for k, ms in zip(some, lists) for m in ms])
    kside = np.concatenate([np.full(len(ms), 1 - int(hs[k]), np.uint8) for k, ms in zip(some, lists)])
    kv = tb.probe(kids, kside)[0].cpu().numpy()
    at = 0
    for k, ms in zip(some, lists):
        first = [m for m, u in zip(ms, kv[at:at + len(ms)]) if int(u) == int(hw[k])][0]
        assert first == int(hl[k]), (k, first, int(hl[k]))
        at += len(ms)
    print("%d children of %d positions probed for the list order" % (len(kids), len(some)))


def test_boards_of_ten_slots(tb, torch):
    """KAABB-KAABB, 243 101 250 entries: no table, cz_tb_boards alone, on the indices the CPU test ranks and unranks"""
    sig = "KAABB-KAABB"
    idx = TC.sample_indices(sig)
    assert len(idx) % 64 != 0 and idx.max() == TM.entries(sig) - 1
    boards, side = tb.boards(sig, idx.astype(np.int32))
    boards, side = boards.cpu().numpy(), side.cpu().numpy()
    empty = 0
    for k, i in enumerate(idx):
        b, s = TM.unrank(sig, int(i))
        assert s == side[k] and np.array_equal(boards[k], np.zeros(90, np.uint8) if b is None else b), (k, i)
        empty += b is None
    print("%s: %d indices, %d of them overlapping" % (sig, len(idx), empty))
    assert 0 < empty < len(idx)
