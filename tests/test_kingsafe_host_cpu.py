"""cz_kingsafe.h (the king-safe move generator cz_movegen_kingsafe runs: one lane = one position) compiled for the HOST and
held, on the CPU, to tests/kingsafe_model.py: the ordered list, the count, the 2086-bit set and the position flags, bit for
bit, on the golden positions, on open boards and on random playouts that go on until a king falls.  The shares of positions in
check, with an unsafe pseudo-legal move, without a safe move and with a king to take are asserted, so that a corpus cannot
quietly become trivial; tests/test_hip_kingsafe.py then pins the kernel around the same function."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kingsafe_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kingsafe") / "libkingsafe_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "kingsafe_host.cpp")])
    lib = C.CDLL(so)
    from oracle import oracle as O
    lut = np.ascontiguousarray(O.lut(), np.int16)
    tab = (C.c_uint8 * lib.czk_host_sizeof_tables())()
    lib.czk_host_tables(lut.ctypes.data_as(C.c_void_p), tab)

    def run(boards, side, want_list=True):
        boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 90)
        side = np.ascontiguousarray(side, np.uint8)
        n = len(boards)
        mv = np.zeros((n, 128), np.uint16)
        c = np.zeros(n, np.int32)
        m = np.zeros((n, 66), np.uint32)
        f = np.zeros(n, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lib.czk_host_kingsafe(tab, p(boards), p(side), n, 1 if want_list else 0, p(mv), p(c), p(m), p(f))
        return mv, c, m, f
    return run


def _hold_to_model(host, boards, side):
    """Every position of the corpus, none left out; -> the model's shares"""
    lists, counts, masks, flags, pseudo = M.model_batch(boards, side)
    mv, c, m, f = host(boards, side)
    assert not (c < 0).any(), np.nonzero(c < 0)[0][:5]          # no position of these corpora is refused
    for i in range(len(boards)):
        assert c[i] == counts[i], (i, c[i], counts[i])
        assert np.array_equal(mv[i, :c[i]], lists[i]), (i, mv[i, :c[i]], lists[i])
        assert (mv[i, c[i]:] == 0xFFFF).all(), i
        assert f[i] == flags[i], (i, f[i], flags[i])
    assert np.array_equal(m, masks), np.nonzero((m != masks).any(axis=1))[0][:5]
    _, c0, _, f0 = host(boards, side, want_list=False)            # the flags-only form gives the same flags and count
    assert np.array_equal(c0, c) and np.array_equal(f0, f)
    return M.shares(counts, flags, pseudo)


def test_golden_positions(host, rules_golden):
    g = rules_golden
    assert len(g["boards"]) == 4381
    check, differs, mated, takes = _hold_to_model(host, g["boards"], g["side"])
    print("golden: in check %d, king-safe != pseudo-legal %d, no safe move %d, can take the king %d" % (check, differs, mated, takes))
    assert check >= 500 and differs >= 1400 and mated >= 30 and takes >= 500


def test_open_boards(host):
    from conftest import open_boards
    boards, side = open_boards(900, 12)
    check, differs, mated, takes = _hold_to_model(host, boards, side)
    print("open boards: in check %d, king-safe != pseudo-legal %d, no safe move %d, can take the king %d" % (check, differs, mated, takes))
    assert check >= 120 and differs >= 350 and mated >= 1 and takes >= 400


def test_random_playouts_until_a_king_falls(host):
    boards, side = M.playout_corpus()
    assert len(boards) >= 5000
    check, differs, mated, takes = _hold_to_model(host, boards, side)
    print("playouts: %d positions, in check %d, king-safe != pseudo-legal %d, no safe move %d, can take the king %d" % (len(boards), check, differs, mated, takes))
    assert check >= 500 and differs >= 1500 and mated >= 10     # measured with the model: about an eighth in check, a third with an unsafe move
    assert ((boards == 1).sum(axis=1) == 0).any() or ((boards == 8).sum(axis=1) == 0).any()   # positions without a king are in


def test_boards_the_generators_refuse_answer_minus_one(host):
    """A third rook of the side to move: count -1 (0xFFFF through the C ABI) and flags 0, as czm_position / czm_list refuse it;
    the same piece of the side not to move is an ordinary attacker."""
    from oracle import oracle as O
    b = O.fen_to_board(O.START_FEN)
    b[4 * 9 + 4] = 3
    mv, c, m, f = host(np.stack([b, b]), np.array([0, 1], np.uint8))
    assert c[0] == -1 and f[0] == 0
    lists, counts, masks, flags, _ = M.model_batch([b], [1])
    assert c[1] == counts[0] and f[1] == flags[0] and np.array_equal(mv[1, :c[1]], lists[0]) and np.array_equal(m[1], masks[0])
