"""cz_chase.h (the threat analysis cz_threats runs: one lane = one position) compiled for the HOST and held, on the CPU, to
tests/chase_model.py bit for bit: the table of constructed positions, random playouts and the golden rules positions.  The
share of positions with a threat is asserted so that the corpus cannot quietly become trivial.  The same source, built as a
stand-alone program with AddressSanitizer and UBSan, runs over the playout corpus; and czk_attacked, which the analysis
extends by a parameter, is held to the model of the king-safe generator for the callers it had before."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chase_cases as CC
import chase_model as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "chase_host.cpp")
_p = lambda a: a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("chase") / "libchase_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    from oracle import oracle as O
    lut = np.ascontiguousarray(O.lut(), np.int16)
    tab = (C.c_uint8 * lib.czc_host_sizeof_tables())()
    lib.czc_host_tables(_p(lut), tab)

    def run(boards, side):
        boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, 90)
        side = np.ascontiguousarray(side, np.uint8)
        out = np.full((len(boards), 4), 0x5A5A, np.uint64)
        ok = np.zeros(len(boards), np.uint8)
        lib.czc_host_threats(tab, _p(boards), _p(side), len(boards), _p(out), _p(ok))
        return out, ok
    run.lib, run.tab = lib, tab
    return run


def _hold(host, ref):
    boards, side, recs = ref
    out, ok = host(boards, side)
    assert ok.all(), np.nonzero(ok == 0)[0][:5]
    bad = np.nonzero((out != recs).any(axis=1))[0]
    assert len(bad) == 0, (bad[:5], out[bad[:2]], recs[bad[:2]])
    return int(((recs[:, 0] | recs[:, 1]) != 0).sum())


def test_table(host):
    _hold(host, CM.table_reference())
    out, _ = host(np.stack([c[1] for c in CC.TABLE]), [c[2] for c in CC.TABLE])
    for (name, _, _, want), row in zip(CC.TABLE, out):
        assert int(row[0]) | (int(row[1]) << 64) == CM.bits(want), name
    boards = np.stack([CM.mirror(c[1]) for c in CC.TABLE])                    # the other colour
    out, _ = host(boards, [1 - c[2] for c in CC.TABLE])
    for (name, _, _, want), row in zip(CC.TABLE, out):
        assert int(row[0]) | (int(row[1]) << 64) == CM.bits([CM.mirror_sq(q) for q in want]), name


def test_constructed_line(host):
    for mirrored in (False, True):
        boards, sides, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE, mirrored)
        out, ok = host(boards, sides)
        assert ok.all() and np.array_equal(out, CM.records(boards, sides))


def test_random_playouts(host):
    ref = CM.corpus_reference()
    assert len(ref[0]) >= 5000
    nonempty = _hold(host, ref)
    print("playouts: %d of %d positions have a threatened piece" % (nonempty, len(ref[0])))
    assert nonempty >= 0.25 * len(ref[0])            # the 12-game subset measured 50 %


def test_golden_positions(host, rules_golden):
    ref = CM.golden_reference(rules_golden)
    assert len(ref[0]) == 4381
    nonempty = _hold(host, ref)
    print("golden: %d of 4381 positions have a threatened piece" % nonempty)
    assert nonempty >= 400


def test_a_board_that_is_not_a_set_answers_four_zero_words(host):
    from oracle import oracle as O
    b = O.fen_to_board(O.START_FEN)
    b[4 * 9 + 4] = 3                                  # a third red rook
    out, ok = host(np.stack([b, b]), [0, 1])
    assert not ok.any() and (out == 0).all()


def test_sanitized_stand_alone_program(host, tmp_path):
    """-fsanitize=address,undefined on a program with its own main, over the playout corpus: it must end clean and write the
    model's records."""
    from oracle import oracle as O
    exe = str(tmp_path / "chase_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCHASE_HOST_MAIN",
                           "-o", exe, SRC])
    boards, side, recs = CM.corpus_reference()
    np.ascontiguousarray(O.lut(), np.int16).tofile(str(tmp_path / "lut"))
    boards.tofile(str(tmp_path / "boards")); side.tofile(str(tmp_path / "side"))
    r = subprocess.run([exe, str(tmp_path / "lut"), str(tmp_path / "boards"), str(tmp_path / "side"), str(tmp_path / "out")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert np.array_equal(np.fromfile(str(tmp_path / "out"), np.uint64).reshape(-1, 4), recs)


def test_czk_attacked_is_unchanged_for_kings_and_exact_for_any_square(host):
    """The default czk_attacked on a king's square is kingsafe_model.attacked (today's callers); czk_attacked(fly = false) on ANY
    square that the other side holds (a cannon needs its target occupied) is 'the attacker has a pseudo-legal move
    onto it', flying general excluded."""
    from kingsafe_model import attacked
    from oracle import oracle as O
    boards, side, _ = CM.corpus_reference()
    boards, side = boards[::7], side[::7]
    srcdst = O.label_srcdst().astype(np.int64)
    bs, as_, ks, fly, want = [], [], [], [], []
    for b, s in zip(boards, side):
        for victim in (0, 1):
            king = np.nonzero(b == (8 if victim else 1))[0]
            if len(king):
                bs.append(b); as_.append(1 - victim); ks.append(king[0]); fly.append(1); want.append(attacked(b, victim))
        s = int(s)
        mv = O.legal_moves(b, s)
        dst, src = srcdst[mv] >> 8, srcdst[mv] & 0xFF
        kq = np.nonzero(b == (8 if s else 1))[0]
        ek = np.nonzero(b == (1 if s else 8))[0]
        fly_move = lambda a, d: len(kq) and len(ek) and a == kq[0] and d == ek[0] and abs(int(d) - int(a)) > 9
        hit = set(int(d) for a, d in zip(src, dst) if not fly_move(a, d))
        own = (b >= 8) if s else ((b >= 1) & (b <= 7))
        for k in np.nonzero(~own & (b != 0))[0]:
            bs.append(b); as_.append(s); ks.append(k); fly.append(0); want.append(int(k) in hit)
    bs, as_, ks, fly = np.stack(bs), np.array(as_, np.uint8), np.array(ks, np.uint8), np.array(fly)
    got = np.zeros(len(bs), np.uint8)
    for f in (0, 1):
        sel = np.nonzero(fly == f)[0]
        o = np.zeros(len(sel), np.uint8)
        host.lib.czc_host_attacked(host.tab, _p(np.ascontiguousarray(bs[sel])), _p(np.ascontiguousarray(as_[sel])), _p(np.ascontiguousarray(ks[sel])), len(sel), f, _p(o))
        got[sel] = o
    want = np.array(want, np.uint8)
    assert (fly == 1).sum() >= 1500 and (fly == 0).sum() >= 5000 and want[fly == 0].sum() >= 1000
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
