"""Model-free identities of the endgame tablebases (TEST INFRASTRUCTURE), shared by tests/test_tablebase_classes_cpu.py (the host
build of cz_tablebase.h) and tests/test_hip_tablebase_classes.py (the kernels).  tests/tablebase_model.py is too slow for tables
with the red advisor / elephant domains, with two equal pieces on a large domain or with more than five slots, so those are held
to what needs no model:
    flip       ranks reversed, colours swapped, side swapped: the same game seen from the other side.  A value is from the mover's
               view, so table[b][rank(flip(board))] == table[a][index] for a = "KR-KAB", b = "KAB-KR"
    mirror     files reversed, side kept: the same inside one table
    canonical  among equal pieces the k-th in ascending square order ranks to the k-th slot; every other arrangement of them is an
               index of its own that must hold the same value
    fixpoint   every value is the pass rule on its children's FINAL values (pass_rule; the children by movegen_kingsafe ->
               successors -> probe, none of which the build uses)
and to PINNED: passes, counts, longest lines and crc32 of four tables as the HOST build of the header computes them, sequentially
and in place (tests/test_tablebase_classes_cpu.py re-measures them on every run; the GPU tables are held to the same numbers).  A
fixpoint alone cannot see a build that stopped too early — deep wins left as draws are a fixpoint too —, the pinned numbers can.

The identities are written once over a SOURCE of tables: an object with
    table(sig)                int16 tensor [entries]
    boards(sig, index)        index int64 tensor [G] -> (boards u8 [G, 90], side u8 [G]); an index whose slots overlap: an empty board
    rank(sig, boards, side)   -> int64 tensor [G]: the index of every position, -1 where it has none
HostTables (ctypes on tests/tablebase_host.cpp) and DeviceTables (a cchess_zero_amd.tablebase.Tablebase) are the two."""
import ctypes as C
import zlib

import numpy as np
import torch

ILLEGAL = -32768
CHUNK = 1 << 20

# The host build of cz_tablebase.h: every index in ascending order, in place, the stop rule of include/cchess_hip.h
PINNED = {
    "KR-KAB": dict(entries=510300, passes=17, legal=285774, wins=128664, losses=148410, longest_win=15, longest_loss=16, crc32=0xA94A589E),
    "KAB-KR": dict(entries=510300, passes=17, legal=285774, wins=128664, losses=148410, longest_win=15, longest_loss=16, crc32=0x0B0707C1),
    "KPP-K": dict(entries=490050, passes=21, legal=309474, wins=141606, losses=159768, longest_win=19, longest_loss=20, crc32=0xCED5583D),
    "K-KPP": dict(entries=490050, passes=21, legal=309474, wins=141606, losses=159768, longest_win=19, longest_loss=20, crc32=0x352F35DB),
}
NON_CANONICAL = {"KPP-K": 231822, "K-KPP": 231822}   # indices with both pawns apart and the higher square on the first slot

_FLIP = [9 * (9 - q // 9) + q % 9 for q in range(90)]
_MIRROR = [9 * (q // 9) + 8 - q % 9 for q in range(90)]


def flip(boards, side):
    """y -> 9 - y, piece codes 1 .. 7 <-> 8 .. 14, side -> 1 - side"""
    b = boards[:, torch.tensor(_FLIP, device=boards.device)]
    return torch.where(b == 0, b, torch.where(b <= 7, b + 7, b - 7)), 1 - side


def mirror(boards):
    """x -> 8 - x"""
    return boards[:, torch.tensor(_MIRROR, device=boards.device)]


def sample_indices(sig, n=4000):
    """n seeded random indices of a signature and the four at its ends (int64 array): 4 004 is no multiple of 64"""
    import tablebase_model as TM
    e = TM.entries(sig)
    rng = np.random.default_rng(sum(sig.encode()))
    return np.concatenate([rng.integers(0, e, n), [0, 1, e - 2, e - 1]]).astype(np.int64)


def has_equal_pieces(sig):
    return any(h.count(c) > 1 for h in sig.split("-") for c in h)


def table_stats(values, passes):
    """What PINNED records, of int16 values (a tensor or an array)"""
    v = values.cpu().numpy() if torch.is_tensor(values) else np.asarray(values)
    assert v.dtype == np.int16
    w = v.astype(np.int64)
    legal = w != ILLEGAL
    win, loss = legal & (w > 0), legal & (w < 0)
    return dict(entries=int(w.size), passes=int(passes), legal=int(legal.sum()), wins=int(win.sum()), losses=int(loss.sum()),
                longest_win=int(w[win].max()) - 1 if win.any() else -1, longest_loss=-int(w[loss].min()) - 1 if loss.any() else -1,
                crc32=zlib.crc32(np.ascontiguousarray(v).tobytes()))


def _all_indices(src, sig):
    t = src.table(sig)
    return torch.arange(t.numel(), dtype=torch.int64, device=t.device)


def _check_image(src, a, b, image, index, what):
    """Every index of `a` (or those given): a legal one has a board; the image of every board has an index in b, and b holds there
    what a holds here — the value of a legal index, ILLEGAL for an illegal one whose slots do not overlap -> counts"""
    ta, tb = src.table(a), src.table(b)
    index = _all_indices(src, a) if index is None else index.to(torch.int64)
    seen = dict(indices=int(index.numel()), apart=0, legal=0)
    for part in index.split(CHUNK):
        boards, side = src.boards(a, part)
        apart = (boards != 0).any(1)
        va = ta[part]
        lost = ((va != ILLEGAL) & ~apart).nonzero().flatten()
        assert lost.numel() == 0, "%s %s: a legal index whose slots overlap: %s" % (what, a, part[lost[:5]].tolist())
        ib, isd = image(boards[apart], side[apart])
        j = src.rank(b, ib.contiguous(), isd.contiguous())
        none = (j < 0).nonzero().flatten()
        assert none.numel() == 0, "%s %s -> %s: the image has no index: %s" % (what, a, b, part[apart][none[:5]].tolist())
        vb, va = tb[j], va[apart]
        bad = (vb != va).nonzero().flatten()
        assert bad.numel() == 0, "%s %s -> %s: %d of %d values differ, first at %s -> %s: %s against %s" % (
            what, a, b, bad.numel(), va.numel(), part[apart][bad[:5]].tolist(), j[bad[:5]].tolist(), va[bad[:5]].tolist(), vb[bad[:5]].tolist())
        seen["apart"] += int(apart.sum())
        seen["legal"] += int((va != ILLEGAL).sum())
    return seen


def check_flip(src, a, b, index_a=None, index_b=None):
    """a and b name the same material with the colours swapped ("KR-KAB", "KAB-KR"): both ways -> the counts of a"""
    assert a.split("-") == b.split("-")[::-1]
    seen = _check_image(src, a, b, flip, index_a, "flip")
    back = _check_image(src, b, a, flip, index_b, "flip")
    if index_a is None and index_b is None:
        assert seen == back, (seen, back)
    print("flip %s <-> %s: %s" % (a, b, seen))
    return seen


def check_mirror(src, sig, index=None):
    seen = _check_image(src, sig, sig, lambda boards, side: (mirror(boards), side), index, "mirror")
    print("mirror %s: %s" % (sig, seen))
    return seen


def check_canonical(src, sig, index=None):
    """table[rank(board of i)] == table[i] for every i whose slots do not overlap -> how many of them are not their own rank:
    none without equal pieces, some with"""
    t = src.table(sig)
    index = _all_indices(src, sig) if index is None else index.to(torch.int64)
    apart_n = other = 0
    for part in index.split(CHUNK):
        boards, side = src.boards(sig, part)
        apart = (boards != 0).any(1)
        at = part[apart]
        j = src.rank(sig, boards[apart].contiguous(), side[apart].contiguous())
        assert bool((j >= 0).all()), "canonical %s: a board of the table has no index: %s" % (sig, at[(j < 0).nonzero().flatten()[:5]].tolist())
        again = src.rank(sig, *[x.contiguous() for x in src.boards(sig, j)])
        assert torch.equal(again, j), "canonical %s: the rank of a ranked board moves again" % sig
        bad = (t[j] != t[at]).nonzero().flatten()
        assert bad.numel() == 0, "canonical %s: %d values differ from their canonical entry's, first at %s -> %s: %s against %s" % (
            sig, bad.numel(), at[bad[:5]].tolist(), j[bad[:5]].tolist(), t[at][bad[:5]].tolist(), t[j][bad[:5]].tolist())
        apart_n += int(apart.sum())
        other += int((j != at).sum())
    print("canonical %s: %d indices, %d apart, %d of them non-canonical" % (sig, index.numel(), apart_n, other))
    assert (other > 0) == has_equal_pieces(sig), (sig, other)
    return other


def pass_rule(u, par, cnt):
    """The values of n parents from their children's FINAL values (cz_tablebase.h's cztb_step with every child settled): u [T]
    the children's values, par [T] the parent of each, cnt [n] the number of children of every parent -> int64 [n]:
    some child lost -> the fewest plies + 2; every child won -> -(the most plies + 2); no child -> -1; else 0"""
    u, par = u.to(torch.int64), par.to(torch.int64)
    n, big = cnt.shape[0], 1 << 20
    lost = torch.full((n,), big, dtype=torch.int64, device=u.device).scatter_reduce_(0, par, torch.where(u < 0, -u - 1, big), "amin")
    all_won = torch.ones(n, dtype=torch.int64, device=u.device).scatter_reduce_(0, par, (u > 0).to(torch.int64), "amin")
    won = torch.full((n,), -1, dtype=torch.int64, device=u.device).scatter_reduce_(0, par, torch.where(u > 0, u - 1, -1), "amax")
    want = torch.where(lost < big, lost + 2, torch.where((all_won == 1) & (cnt > 0), -(won + 2), torch.zeros_like(lost)))
    return torch.where(cnt == 0, torch.full_like(want, -1), want)


def check_fixpoint(tb, sig, index, chunk=1 << 16):
    """index: legal indices of a built table of tb (a Tablebase).  Every value is the pass rule on the children's final values, the
    children made by cz_tb_boards -> movegen_kingsafe -> successors -> probe; every -1 entry, and no other, has no king-safe
    move; every child is covered.  chunk: parents per batch (a parent has up to ~40 children of 90 bytes) -> counts"""
    from cchess_zero_amd._lib import POS_CAN_TAKE_KING, POS_NO_SAFE_MOVE
    table = tb.tables[sig]
    seen = dict(parents=0, children=0, batches=0)
    for part in index.to(torch.int64).split(chunk):
        boards, side = tb.boards(sig, part.to(torch.int32))
        v = table[part].to(torch.int32)
        assert not bool((v == ILLEGAL).any())
        mv, cnt, _, pf = tb.rules.movegen_kingsafe(boards, side, want_mask=False, pad=False)
        assert bool((cnt >= 0).all()) and not bool((pf & POS_CAN_TAKE_KING).any())
        assert torch.equal(v == -1, (pf & POS_NO_SAFE_MOVE) != 0)
        cb, cs, _, par, _ = tb.rules.successors(boards, side, mv, cnt)
        u, covered = tb.probe(cb, cs)
        assert bool(covered.all())
        want = pass_rule(u, par, cnt)
        bad = (want != v.to(torch.int64)).nonzero().flatten()
        assert bad.numel() == 0, (sig, int(bad.numel()), part[bad[:5]], v[bad[:5]], want[bad[:5]])
        seen["parents"] += int(part.numel())
        seen["children"] += int(cb.shape[0])
        seen["batches"] += 1
        del cb, cs, u, par, mv
    print("fixpoint %s: %s" % (sig, seen))
    return seen


def check_illegal(tb, sig, index):
    """index: ILLEGAL indices of a built table.  Two slots share a square (an empty board), or the mover can take the king, or
    the board is refused -> (with all pieces apart, overlapping)"""
    from cchess_zero_amd._lib import POS_CAN_TAKE_KING
    n = len(sig) - 1
    ib, is_ = tb.boards(sig, index.to(torch.int32))
    pieces = (ib != 0).sum(1)
    apart = pieces == n
    assert bool((pieces[~apart] == 0).all())
    _, icnt, _, ipf = tb.rules.movegen_kingsafe(ib[apart].contiguous(), is_[apart].contiguous(), want_mask=False, want_moves=False)
    assert bool((((ipf & POS_CAN_TAKE_KING) != 0) | (icnt < 0)).all())
    print("illegal %s: %d apart, %d overlapping" % (sig, int(apart.sum()), int((~apart).sum())))
    return int(apart.sum()), int((~apart).sum())


_p = lambda a: a.ctypes.data_as(C.c_void_p)


class HostTables:
    """The source on tests/tablebase_host.cpp's library: lib (ctypes), lut and srcdst as test_tablebase_host_cpu.py's `tables`"""

    def __init__(self, lib, lut, srcdst):
        self.lib, self.lut, self.srcdst = lib, lut, srcdst
        self.tables, self.passes = {}, {}

    def entries(self, sig):
        n, e = C.c_int32(), C.c_uint32()
        code, dom, radix = (np.zeros(10, np.uint8) for _ in range(3))
        assert self.lib.cztb_host_parse(sig.encode(), C.byref(n), C.byref(e), _p(code), _p(dom), _p(radix)) == 0
        return int(e.value)

    def build(self, sig):
        values, n_pass = np.zeros(self.entries(sig), np.int16), C.c_int32()
        assert self.lib.cztb_host_build(_p(self.lut), _p(self.srcdst), sig.encode(), _p(values), C.byref(n_pass)) == values.size
        self.tables[sig], self.passes[sig] = torch.from_numpy(values), int(n_pass.value)
        return table_stats(values, n_pass.value)

    def table(self, sig):
        return self.tables[sig]

    def boards_np(self, sig, index):
        index = np.ascontiguousarray(index, np.uint32)
        G = index.size
        boards, side, overlap = np.full((G, 90), 77, np.uint8), np.full(G, 77, np.uint8), np.full(G, 77, np.uint8)
        assert self.lib.cztb_host_boards(sig.encode(), _p(index), G, _p(boards), _p(side), _p(overlap)) == 0
        return boards, side, overlap

    def rank_np(self, sig, boards, side):
        boards, side = np.ascontiguousarray(boards, np.uint8), np.ascontiguousarray(side, np.uint8)
        G = side.size
        status, index = np.full(G, 99, np.int16), np.zeros(G, np.uint32)
        assert self.lib.cztb_host_rank(sig.encode(), _p(boards), _p(side), G, _p(status), _p(index)) == 0
        return status, index

    def boards(self, sig, index):
        boards, side, overlap = self.boards_np(sig, index.numpy())
        assert np.array_equal(overlap != 0, ~(boards != 0).any(1))
        return torch.from_numpy(boards), torch.from_numpy(side)

    def rank(self, sig, boards, side):
        status, index = self.rank_np(sig, boards.numpy(), side.numpy())
        return torch.from_numpy(np.where(status == 0, index.astype(np.int64), -1))


class DeviceTables:
    """The source on a Tablebase: cz_tb_boards and cz_tb_probe (whose value must be the table's at the index it reports)"""

    def __init__(self, tb):
        self.tb = tb

    def table(self, sig):
        return self.tb.tables[sig]

    def boards(self, sig, index):
        return self.tb.boards(sig, index.to(torch.int32))

    def rank(self, sig, boards, side):
        value, index = self.tb.probe_one(sig, boards, side, want_index=True)
        index = index.to(torch.int64)
        found = index >= 0
        assert torch.equal(value[found], self.tb.tables[sig][index[found]]), "cz_tb_probe %s: a value that is not the table's at the index reported" % sig
        return index
