"""cz_tablebase.h (the index mapping and the per-index pass that k_tb_pass, k_tb_probe and k_tb_boards run: one lane = one index)
compiled for the HOST and held, on the CPU, to tests/tablebase_model.py: rank / unrank over every index of K-K, KP-K and
KR-KAA, and cztb_step iterated in place to the recorded K-K, KP-K, KN-K and KN-KA tables, bit for bit.  The same source, built
as a stand-alone program with AddressSanitizer and UBSan, builds KP-K and KN-KA and must end clean with the same tables."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tablebase_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tablebase_host.cpp")
_p = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tablebase") / "libtablebase_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.cztb_host_build.restype = C.c_longlong
    return lib


@pytest.fixture(scope="module")
def tables():
    from oracle import oracle as O
    return np.ascontiguousarray(O.lut(), np.int16), np.ascontiguousarray(O.label_srcdst(), np.uint16)


def test_signatures(host):
    n, e = C.c_int32(), C.c_uint32()
    code, dom, radix = (np.zeros(10, np.uint8) for _ in range(3))
    assert host.cztb_host_parse(b"KR-KAA", C.byref(n), C.byref(e), _p(code), _p(dom), _p(radix)) == 0
    assert (n.value, e.value) == (5, 364500) and list(code[:5]) == [1, 3, 8, 9, 9] and list(radix[:5]) == [9, 90, 9, 5, 5] and list(dom[:5]) == [1, 0, 5, 6, 6]
    for sig in ("K-K", "KP-KP", "KRN-KR", "KCP-KNB", "KAABB-KAABB"):
        assert host.cztb_host_parse(sig.encode(), C.byref(n), C.byref(e), _p(code), _p(dom), _p(radix)) == 0
        assert e.value == TM.entries(sig) and n.value == len(TM.parse(sig))
        assert [int(c) for c in code[:n.value]] == [c for c, _ in TM.parse(sig)] and [int(r) for r in radix[:n.value]] == [len(d) for _, d in TM.parse(sig)]
    for bad in ("", "K", "K-", "-K", "R-K", "KK-K", "KRK-K", "KAR-K", "KRRR-K", "KPPPPPP-K", "K-K-K", "KX-K", "k-k", "KRR-KRR", "KAABBP-KAABB"):
        assert host.cztb_host_parse(bad.encode(), C.byref(n), C.byref(e), _p(code), _p(dom), _p(radix)) < 0, bad


@pytest.mark.parametrize("sig", ["K-K", "KP-K", "KR-KAA"])
def test_rank_and_unrank_over_every_index(host, sig):
    """Every index: the board and side of the model's unrank (an empty board for an overlap); every board ranks back to the
    model's canonical index, which for two equal pieces is the index itself only when they stand in ascending order"""
    n = TM.entries(sig)
    slots = TM.parse(sig)
    idx = np.arange(n, dtype=np.uint32)
    boards, side, overlap = np.full((n, 90), 77, np.uint8), np.full(n, 77, np.uint8), np.full(n, 77, np.uint8)
    assert host.cztb_host_boards(sig.encode(), _p(idx), n, _p(boards), _p(side), _p(overlap)) == 0
    # the model's unrank, vectorised from its definition: digits from the least significant slot, squares from the domains
    m = idx.astype(np.int64) >> 1
    want = np.zeros((n, 90), np.uint8)
    count = np.zeros((n, 90), np.uint8)
    sq = []
    for code, d in reversed(slots):
        q = d[m % len(d)]
        m //= len(d)
        want[np.arange(n), q] = code
        count[np.arange(n), q] += 1
        sq.append(q)
    ov = (count > 1).any(1)
    want[ov] = 0
    assert np.array_equal(overlap, ov.astype(np.uint8)) and np.array_equal(side, (idx & 1).astype(np.uint8)) and np.array_equal(boards, want)
    for i in range(0, n, max(1, n // 300)):            # the vectorised restatement against the model's own function
        b, s = TM.unrank(sig, i)
        assert (b is None) == bool(ov[i]) and (b is None or np.array_equal(b, want[i])) and s == side[i]
    status, back = np.full(n, 99, np.int16), np.zeros(n, np.uint32)
    assert host.cztb_host_rank(sig.encode(), _p(boards), _p(side), n, _p(status), _p(back)) == 0
    assert (status[ov] == TM.MISS).all() and (status[~ov] == 0).all()               # an empty board has other pieces than the signature's
    # the canonical index: equal pieces sorted by square.  Only KR-KAA has two: slots 3 and 4
    canon = idx.astype(np.int64)
    if sig == "KR-KAA":
        a2, a1 = sq[0], sq[1]                                                       # slot 4, slot 3 (reversed order above)
        d1, d2 = (idx >> 1) // 5 % 5, (idx >> 1) % 5
        swap = a1 > a2
        canon = np.where(swap, idx.astype(np.int64) + 2 * ((d2.astype(np.int64) - d1) * 5 + (d1.astype(np.int64) - d2)), canon)
        assert swap[~ov].any() and (~swap[~ov]).any()
    assert np.array_equal(back[~ov].astype(np.int64), canon[~ov])
    for i in np.nonzero(~ov)[0][::max(1, n // 300)]:
        assert TM.rank(sig, boards[i], int(side[i])) == int(back[i])
    # foreign boards, a piece outside its domain, a byte that is no piece code
    fb, fs = boards[~ov][:3].copy(), side[~ov][:3].copy()
    fb[0, np.nonzero(fb[0] == 1)[0][0]] = 0
    fb[0, 0 if fb[0, 0] == 0 else 1] = 1                                            # the red king on a1 or b1: outside the palace
    fb[1, np.nonzero(fb[1] == 0)[0][0]] = 14                                        # one piece more
    fb[2, np.nonzero(fb[2] == 0)[0][0]] = 200
    st3, ix3 = np.zeros(3, np.int16), np.zeros(3, np.uint32)
    host.cztb_host_rank(sig.encode(), _p(fb), _p(fs), 3, _p(st3), _p(ix3))
    assert list(st3) == [TM.ILLEGAL, TM.MISS, TM.MISS]


@pytest.mark.parametrize("sig", ["K-K", "KP-K", "KN-K", "KN-KA"])
def test_the_step_iterated_on_the_host_builds_the_recorded_tables(host, tables, sig):
    """cztb_step over every index, pass after pass, IN PLACE as k_tb_pass runs it (the model's passes are synchronous), with the
    header's stop rule: the model's table and its number of passes"""
    values, passes = TM.golden()
    got, n_pass = np.zeros(TM.entries(sig), np.int16), C.c_int32()
    assert host.cztb_host_build(_p(tables[0]), _p(tables[1]), sig.encode(), _p(got), C.byref(n_pass)) == TM.entries(sig)
    bad = np.nonzero(got != values[sig])[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:5]], values[sig][bad[:5]])
    assert n_pass.value == passes[sig]
    assert host.cztb_host_build(_p(tables[0]), _p(tables[1]), b"KR-KK", _p(got), C.byref(n_pass)) < 0


def test_sanitized_stand_alone_program(tmp_path, tables):
    """-fsanitize=address,undefined on a program with its own main: it builds KP-K and KN-KA (their closures on the way), checks
    the rank / unrank round trip of every index, must end clean and write the recorded tables"""
    exe = str(tmp_path / "tablebase_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DTABLEBASE_HOST_MAIN",
                           "-o", exe, SRC])
    tables[0].tofile(str(tmp_path / "lut"))
    tables[1].tofile(str(tmp_path / "srcdst"))
    r = subprocess.run([exe, str(tmp_path), "KP-K", "KN-KA"], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert "0 round-trip failures" in r.stdout
    values, _ = TM.golden()
    for sig in ("KP-K", "KN-KA"):
        assert np.array_equal(np.fromfile(str(tmp_path / sig), np.int16), values[sig])
