"""SearchEngine.xcache_dump against a stub library: the raw block of cz_search_debug_xcache_dump, built here from the offsets
include/cchess_hip.h documents (they are the ABI, so they stand as literals), comes back field by field.  No GPU."""
import ctypes as C

import numpy as np

from cchess_zero_amd import _lib, engine

N = 64   # the smallest table (cz_search_set_xcache(6))
# include/cchess_hip.h: key u64 [n] | 64 bytes | value f32 [n] | count | ply << 16 u32 [n] | packed position u32 [n][12] |
# labels u16 [n][128] | (src | dst << 8) u16 [n][128] | priors f32 [n][128]; n * 1088 + 64 bytes
DOCUMENTED = dict(key=(0, np.uint64, 1), value=(N * 8 + 64, np.float32, 1), count_ply=(N * 12 + 64, np.uint32, 1),
                  board=(N * 16 + 64, np.uint32, 12), label=(N * 64 + 64, np.uint16, 128), sd=(N * 320 + 64, np.uint16, 128),
                  P=(N * 576 + 64, np.float32, 128))
TOTAL = N * 1088 + 64


def _fields():
    """Every field of every entry with a value of its own (distinct within the field; the fields differ in type or range)."""
    e = np.arange(N, dtype=np.uint64)
    j = np.arange(128, dtype=np.uint32)
    return dict(key=e * np.uint64(0x0123456789ABCDEF) + np.uint64(1 << 40),
                value=(e.astype(np.float32) + 0.25) / np.float32(-64.0),
                count_ply=((e.astype(np.uint32) + 1) * 2) | ((e.astype(np.uint32) * 3 + 7) << 16),
                board=(e.astype(np.uint32)[:, None] * 12 + j[None, :12]) * np.uint32(0x01000193) + np.uint32(5),
                label=(e.astype(np.uint32)[:, None] * 128 + j[None, :]).astype(np.uint16),
                sd=(0xFFFF - (e.astype(np.uint32)[:, None] * 128 + j[None, :])).astype(np.uint16),
                P=(e.astype(np.float32)[:, None] * 128 + j[None, :].astype(np.float32) + 1) / np.float32(16384.0))


def _raw_block(fields):
    raw = np.full(TOTAL, 0xA5, np.uint8)   # the 64 bytes behind the keys belong to no field
    covered = np.zeros(TOTAL, bool)
    for name, (off, dt, per) in DOCUMENTED.items():
        b = np.ascontiguousarray(fields[name], dt).view(np.uint8).reshape(-1)
        assert b.size == N * per * np.dtype(dt).itemsize and not covered[off:off + b.size].any()
        raw[off:off + b.size] = b
        covered[off:off + b.size] = True
    assert covered.sum() == TOTAL - 64 and not covered[N * 8:N * 8 + 64].any()
    return raw


class StubLib:
    """Stands in for libcchess_hip.so: a cross-tree table of N entries holding `raw`."""

    def __init__(self, raw):
        self.raw = raw
        self.sizes = []

    def cz_last_error(self):
        return b"stub"

    def cz_search_debug_xcache_dump(self, handle, host, nbytes):
        self.sizes.append(nbytes)
        if host is None:
            return N
        if nbytes < self.raw.nbytes:
            return -1
        C.memmove(host, self.raw.ctypes.data, self.raw.nbytes)
        return N


def test_xcache_dump_returns_every_documented_field(monkeypatch):
    fields = _fields()
    for name, a in fields.items():
        assert np.unique(a).size == a.size, name
    stub = StubLib(_raw_block(fields))
    monkeypatch.setattr(_lib, "_lib", stub)
    ctx = engine.Context.__new__(engine.Context)
    ctx.h = C.c_void_p(0x55)
    ctx.bind_stream = lambda: None
    eng = engine.SearchEngine.__new__(engine.SearchEngine)
    eng.ctx = ctx
    try:
        d = eng.xcache_dump()
    finally:
        ctx.h = None   # nothing for __del__ to destroy
    assert stub.sizes == [0, TOTAL]
    assert sorted(d) == sorted(["key", "value", "count", "ply", "board", "label", "sd", "P"])
    for name in ("key", "value", "board", "label", "sd", "P"):
        off, dt, per = DOCUMENTED[name]
        assert d[name].dtype == dt and d[name].shape == ((N, per) if per > 1 else (N,)), name
        assert np.array_equal(d[name], fields[name]), name
    # the count word: the move count in its low half, the game ply in its high half
    assert d["count"].dtype == np.uint16 and d["ply"].dtype == np.uint16
    assert np.array_equal(d["count"], (np.arange(N) + 1) * 2) and np.array_equal(d["ply"], np.arange(N) * 3 + 7)
    # the engine's own table states the documented entry
    assert engine.XC_ENTRY_BYTES == 1088 and engine.XC_COUNTER_BYTES == 64
    assert [(f[0], f[3]) for f in engine.XC_FIELDS] == [("key", 0), ("value", 8), ("count_ply", 12), ("board", 16), ("label", 64), ("sd", 320),
                                                         ("P", 576)]
