"""cz_kingsafe.h's checking-move pass (czk_checks behind czk_filter: what cz_movegen_checks runs, one lane = one position)
compiled for the HOST and held, on the CPU, to tests/mate_model.checks: the ordered list of the king-safe moves that give check,
its count and the position's own flags, bit for bit, on the golden positions, on open boards and on random playouts that go on
until a king falls — no position left out.  That the corpora are not trivial is asserted: positions with a checking move,
discovered checks (the moved piece is not the one that attacks the king) and cannon checks over a screen."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kingsafe_model as M
import mate_model as MM
from perft_model import make_move

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("checks") / "libchecks_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "checks_host.cpp")])
    lib = C.CDLL(so)
    from oracle import oracle as O
    lut = np.ascontiguousarray(O.lut(), np.int16)
    tab = (C.c_uint8 * lib.czc_host_sizeof_tables())()
    lib.czc_host_tables(lut.ctypes.data_as(C.c_void_p), tab)

    def run(boards, side, want_list=True):
        boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 90)
        side = np.ascontiguousarray(side, np.uint8)
        n = len(boards)
        mv = np.zeros((n, 128), np.uint16)
        c = np.zeros(n, np.int32)
        f = np.zeros(n, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lib.czc_host_checks(tab, p(boards), p(side), n, 1 if want_list else 0, p(mv), p(c), p(f))
        return mv, c, f
    return run


def _attackers(board, s):
    """The squares of side s's pieces that have a pseudo-legal move onto the other king (empty without that king)"""
    from oracle import oracle as O
    king = np.nonzero(np.asarray(board) == (1 if s else 8))[0]
    if len(king) == 0:
        return []
    sd = O.label_srcdst().astype(np.int64)[O.legal_moves(board, s)]
    return [int(x) & 0xFF for x in sd if int(x) >> 8 == king[0]]


def _hold_to_model(host, boards, side):
    """Every position of the corpus -> (positions with both kings and no king to take, those of them with a checking move,
    discovered checks, cannon checks) of the model"""
    from oracle import oracle as O
    dst_of = O.label_srcdst().astype(np.int64) >> 8
    mv, c, f = host(boards, side)
    assert not (c < 0).any(), np.nonzero(c < 0)[0][:5]          # no position of these corpora is refused
    legal = with_check = discovered = cannon = 0
    for i in range(len(boards)):
        b, s = boards[i], int(side[i])
        lst, flags = MM.checks(b, s)
        assert c[i] == len(lst), (i, c[i], len(lst))
        assert np.array_equal(mv[i, :c[i]], lst), (i, mv[i, :c[i]], lst)
        assert (mv[i, c[i]:] == 0xFFFF).all(), i
        assert f[i] == flags, (i, f[i], flags)
        if MM.bad_root(b, s):        # a mover that can take the king "checks" with every move that does not stop it
            continue
        legal += 1
        with_check += len(lst) > 0
        for m in lst:
            child = make_move(b, m)[0]
            att = _attackers(child, s)
            assert att
            discovered += int(dst_of[int(m)]) not in att
            cannon += any(child[q] in (7, 14) for q in att)
    _, c0, f0 = host(boards, side, want_list=False)               # the count / flags form gives the same count and flags
    assert np.array_equal(c0, c) and np.array_equal(f0, f)
    return legal, with_check, discovered, cannon


def test_golden_positions(host, rules_golden):
    g = rules_golden
    assert len(g["boards"]) == 4381
    legal, with_check, discovered, cannon = _hold_to_model(host, g["boards"], g["side"])
    print("golden: %d legal roots, %d with a checking move, %d discovered checks, %d cannon checks" % (legal, with_check, discovered, cannon))
    assert legal >= 300 and 5 * with_check >= legal and discovered >= 1 and cannon >= 1   # the playouts' share of roots with a check is 44 %


def test_open_boards(host):
    from conftest import open_boards
    boards, side = open_boards(900, 12)
    legal, with_check, discovered, cannon = _hold_to_model(host, boards, side)
    print("open boards: %d legal roots, %d with a checking move, %d discovered checks, %d cannon checks" % (legal, with_check, discovered, cannon))
    assert legal >= 300 and 5 * with_check >= legal and discovered >= 1 and cannon >= 1


def test_random_playouts_until_a_king_falls(host):
    """Measured with the model: of the 6 272 positions 5 663 have both kings and no king to take, 2 474 of those a checking move."""
    boards, side = M.playout_corpus()
    legal, with_check, discovered, cannon = _hold_to_model(host, boards, side)
    print("playouts: %d positions, %d legal roots, %d with a checking move, %d discovered checks, %d cannon checks" % (len(boards), legal, with_check, discovered, cannon))
    assert len(boards) >= 5000 and with_check >= 2000 and discovered >= 1 and cannon >= 1


def test_a_move_that_takes_the_king_gives_no_check(host):
    """A rook that can take the other king: the capture is king-safe and is no check; the position's flags say CAN_TAKE_KING."""
    b = np.zeros(90, np.uint8)
    b[4], b[9 * 9 + 3], b[5 * 9 + 3] = 1, 8, 3                  # red king e0, black king d9, red rook d5
    lst, flags = MM.checks(b, 0)
    mv, c, f = host(b[None], np.array([0], np.uint8))
    from oracle import oracle as O
    sd = O.label_srcdst().astype(np.int64)
    assert flags & M.CAN_TAKE_KING and f[0] == flags and c[0] == len(lst) and np.array_equal(mv[0, :c[0]], lst)
    assert all(int(sd[int(m)]) >> 8 != 9 * 9 + 3 for m in lst)


def test_boards_the_generators_refuse_answer_minus_one(host):
    """A third rook of the side to move: count -1 (0xFFFF through the C ABI) and flags 0; the same piece of the side not to move
    is an ordinary piece."""
    from oracle import oracle as O
    b = O.fen_to_board(O.START_FEN)
    b[4 * 9 + 4] = 3
    mv, c, f = host(np.stack([b, b]), np.array([0, 1], np.uint8))
    assert c[0] == -1 and f[0] == 0
    lst, flags = MM.checks(b, 1)
    assert c[1] == len(lst) and f[1] == flags and np.array_equal(mv[1, :c[1]], lst)
