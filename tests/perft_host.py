"""tests/perft_host.cpp compiled with g++ and bound with ctypes (TEST INFRASTRUCTURE): the recursive host perft over the
library's own king-safe generator.  tests/golden/gen_perft.py writes the fixture with it, tests/test_perft_cpu.py holds it to
the fixture.  No GPU code is involved."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = ("nodes", "captures", "checks", "mates")


def load(build_dir):
    """Compiles the host perft into build_dir -> perft(board, side, depth, stats=True): a dict of int64 arrays [depth + 1]
    (nodes alone without stats: the last ply is counted from its parents' lists, as Rules.perft does)."""
    so = os.path.join(str(build_dir), "libperft_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "perft_host.cpp")])
    lib = C.CDLL(so)
    from oracle import oracle as O
    lut = np.ascontiguousarray(O.lut(), np.int16)
    srcdst = np.ascontiguousarray(O.label_srcdst(), np.uint16)
    tab = (C.c_uint8 * lib.perft_host_sizeof_tables())()
    lib.perft_host_tables(lut.ctypes.data_as(C.c_void_p), tab)

    def perft(board, side, depth, stats=True):
        board = np.ascontiguousarray(board, np.uint8).reshape(90)
        out = [np.zeros(depth + 1, np.int64) for _ in COLUMNS]
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.perft_host(tab, p(srcdst), p(board), int(side), int(depth), 1 if stats else 0, *[p(a) for a in out])
        if rc != 0:
            raise ValueError("perft_host: a position the generator refuses")
        return dict(zip(COLUMNS, out)) if stats else {"nodes": out[0]}
    return perft
