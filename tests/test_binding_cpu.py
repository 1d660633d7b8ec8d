"""The host binding layer (_lib.call / out_pointers, engine.Context.call / download) against a stub library: no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from cchess_zero_amd import _lib
from cchess_zero_amd.engine import Context


class StubLib:
    """Stands in for libcchess_hip.so: records what every call received."""

    def __init__(self):
        self.calls = []
        self.rc = 0
        self.error = b"stub says no"

    def cz_last_error(self):
        return self.error

    def cz_anything(self, *args):
        self.calls.append(("cz_anything", args))
        return self.rc

    def cz_getter(self, handle, player, *out):
        self.calls.append(("cz_getter", (handle, player)))
        for i, p in enumerate(out):
            p._obj.value = 0x1000 * (i + 1) + player
        return 0

    def cz_set_stream(self, handle, stream):
        self.calls.append(("cz_set_stream", (handle, stream)))
        return 0

    def cz_download(self, handle, dst, src, n):
        self.calls.append(("cz_download", (handle, dst, src, n)))
        C.memmove(dst, src, n)
        return 0


@pytest.fixture
def stub(monkeypatch):
    s = StubLib()
    monkeypatch.setattr(_lib, "_lib", s)
    return s


def test_call_hands_arguments_through(stub):
    t = torch.arange(6, dtype=torch.int32)
    p, n = C.c_void_p(0x1234), C.c_ulonglong(7)
    ref = C.byref(n)
    assert _lib.call("cz_anything", t, None, p, ref, 3, 0.25) == 0
    (name, got), = stub.calls
    assert name == "cz_anything" and got[0] == t.data_ptr() and got[1] is None and got[2] is p and got[3] is ref
    assert got[4] == 3 and type(got[4]) is int and got[5] == 0.25 and type(got[5]) is float


def test_call_returns_a_count(stub):
    stub.rc = 41
    assert _lib.call("cz_anything") == 41


@pytest.mark.parametrize("rc", [-1, -2, -3])
def test_call_raises_with_the_name_and_the_library_text(stub, rc):
    stub.rc = rc
    with pytest.raises(_lib.CchessHipError) as e:
        _lib.call("cz_anything", 1)
    assert "cz_anything failed (%d): stub says no" % rc in str(e.value)


def test_out_pointers_returns_what_the_getter_wrote(stub):
    h = C.c_void_p(0x77)
    ptrs = _lib.out_pointers("cz_getter", h, 3, 1)
    assert [p.value for p in ptrs] == [0x1001, 0x2001, 0x3001] and all(isinstance(p, C.c_void_p) for p in ptrs)
    assert stub.calls == [("cz_getter", (h, 1))]


@pytest.fixture
def ctx(stub):
    """A Context made without a device: a made-up handle and a recording bind_stream."""
    c = Context.__new__(Context)
    c.h = C.c_void_p(0x55)
    c.bind_stream = lambda: stub.calls.append(("bind", ()))
    yield c
    c.h = None   # nothing for __del__ to destroy


def test_context_call_binds_then_prepends_the_handle(stub, ctx):
    stub.rc = 5
    assert ctx.call("cz_anything", 9, None) == 5
    assert stub.calls == [("bind", ()), ("cz_anything", (ctx.h, 9, None))]


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.uint64])
def test_context_download_round_trips(stub, ctx, dtype):
    src = (np.arange(24, dtype=np.uint64) * 0x0101010101010101 + 3).astype(dtype).reshape(4, 6)
    out = ctx.download(C.c_void_p(src.ctypes.data), dtype, (4, 6))
    assert out.dtype == dtype and out.shape == (4, 6) and np.array_equal(out, src) and not np.shares_memory(out, src)
    assert [c[0] for c in stub.calls] == ["bind", "cz_download"] and stub.calls[1][1][0] is ctx.h and stub.calls[1][1][3] == src.nbytes
    assert ctx.download(C.c_void_p(src.ctypes.data), dtype, (4, 6)) is not out
