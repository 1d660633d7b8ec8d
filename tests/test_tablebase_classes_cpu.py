"""cz_tablebase.h compiled for the HOST (tests/tablebase_host.cpp) on the material classes that tests/test_tablebase_host_cpu.py
does not reach: the red advisor and elephant domains, tables that black wins, two and more equal pieces on the 55- and 90-square
domains, six to ten slots, indices up to 1.48 G.
  1. rank / unrank against tests/tablebase_model.py on sampled indices of ten signatures (no table is allocated);
  2. KR-KAB, KAB-KR, KPP-K and K-KPP built on the host: the flip, mirror and canonical identities of tests/tablebase_classes.py
     over every index, and the pinned passes, counts, longest lines and crc32 — which tests/test_hip_tablebase_classes.py then
     asks of the GPU's tables;
  3. KP-KP built on the host is the model's recorded table: the one whose build has an empty pass with decided ones behind it."""
import os
import subprocess
import ctypes as C

import numpy as np
import pytest

import tablebase_classes as TC
import tablebase_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tablebase_host.cpp")

SAMPLED = ("KAB-KR", "KPP-K", "KPPP-K", "K-KPPP", "KNN-K", "KP-KAAB", "KRR-KAA", "KAABB-KAABB", "KPPPP-K", "KAB-KPPP")
HOST_BUILT = ("KR-KAB", "KAB-KR", "KPP-K", "K-KPP")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("tablebase_classes") / "libtablebase_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.cztb_host_build.restype = C.c_longlong
    from oracle import oracle as O
    return TC.HostTables(lib, np.ascontiguousarray(O.lut(), np.int16), np.ascontiguousarray(O.label_srcdst(), np.uint16))


@pytest.fixture(scope="module")
def built(host):
    return {sig: host.build(sig) for sig in HOST_BUILT}


@pytest.mark.parametrize("sig", SAMPLED)
def test_rank_and_unrank_against_the_model(host, sig):
    e = TM.entries(sig)
    assert host.entries(sig) == e
    idx = TC.sample_indices(sig)
    boards, side, overlap = host.boards_np(sig, idx)
    status, back = host.rank_np(sig, boards, side)
    apart = 0
    for k, i in enumerate(idx):
        b, s = TM.unrank(sig, int(i))
        assert s == side[k] and (b is None) == bool(overlap[k]), (sig, i)
        assert np.array_equal(boards[k], np.zeros(90, np.uint8) if b is None else b), (sig, i)
        if b is None:
            assert status[k] == TM.MISS
        else:
            apart += 1
            assert status[k] == 0 and int(back[k]) == TM.rank(sig, b, s), (sig, i, int(back[k]), TM.rank(sig, b, s))
    other = int((back[overlap == 0].astype(np.int64) != idx[overlap == 0]).sum())
    print("%s: %d entries, %d sampled, %d apart, %d of them non-canonical, the largest %d" % (sig, e, len(idx), apart, other, idx.max()))
    assert apart > 500 and (other > 0) == TC.has_equal_pieces(sig)


@pytest.mark.parametrize("sig", tuple(dict.fromkeys(SAMPLED + HOST_BUILT)))
def test_descriptor_without_a_slot(host, sig):
    """ord and mult of every slot from the letters; cztb_without(descriptor, j) is, field by field, the descriptor of the signature
    without that letter — ord of the equal pieces behind slot j included"""
    def desc(s, without):
        n, e, f = C.c_int32(), C.c_uint32(), np.full((5, 10), 99, np.uint8)
        assert host.lib.cztb_host_desc(s.encode(), without, C.byref(n), C.byref(e), f.ctypes.data_as(C.c_void_p)) == 0, (s, without)
        return n.value, e.value, f.tolist()
    n, e, f = desc(sig, -1)
    codes = [c for c, _ in TM.parse(sig)]
    pad = [0] * (10 - n)
    assert (n, e) == (len(codes), TM.entries(sig)) and f[0] == codes + pad and f[2] == [len(d) for _, d in TM.parse(sig)] + [1] * (10 - n)
    assert f[3] == [codes[:k].count(codes[k]) for k in range(n)] + pad and f[4] == [codes.count(c) for c in codes] + pad
    assert f[1][n:] == pad
    dropped = 0
    for j, letter in enumerate(sig.replace("-", "")):
        if letter != "K":
            assert desc(sig, j) == desc(TM.sub_signature(sig, j), -1), (sig, j)
            dropped += 1
    assert dropped == n - 2


@pytest.mark.parametrize("sig", HOST_BUILT)
def test_pinned_constants(built, sig):
    print("%s: %s" % (sig, {k: ("%08x" % v if k == "crc32" else v) for k, v in built[sig].items()}))
    assert built[sig] == TC.PINNED[sig]


@pytest.mark.parametrize("a,b", [("KR-KAB", "KAB-KR"), ("KPP-K", "K-KPP")])
def test_flip(host, built, a, b):
    seen = TC.check_flip(host, a, b)
    assert seen["legal"] == TC.PINNED[a]["legal"] and seen["apart"] > seen["legal"]
    for k in ("passes", "legal", "wins", "losses", "longest_win", "longest_loss"):
        assert built[a][k] == built[b][k]


@pytest.mark.parametrize("sig", HOST_BUILT)
def test_mirror(host, built, sig):
    assert TC.check_mirror(host, sig)["legal"] == TC.PINNED[sig]["legal"]


@pytest.mark.parametrize("sig", ["KPP-K", "K-KPP"])
def test_canonical(host, built, sig):
    assert TC.check_canonical(host, sig) == TC.NON_CANONICAL[sig]


def test_the_stop_rule_on_kp_kp(host):
    """KP-KP's pass 12 decides nothing and passes up to 21 decide again (its sub-tables hold losses of 20 plies): a build that
    stops at the first empty pass ends with 8 538 wins instead of 13 362"""
    values, passes = TM.golden()
    st = host.build("KP-KP")
    assert np.array_equal(host.table("KP-KP").numpy(), values["KP-KP"]) and st["passes"] == passes["KP-KP"] and st["wins"] == 13362
