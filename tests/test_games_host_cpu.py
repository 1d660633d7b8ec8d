"""cz_games.h (the per-game step cz_games_replay runs: one lane = one game) compiled for the HOST and held, on the CPU, to
tests/games_model.py byte for byte: the reference's six self-play games and the fault corpus of tests/games_cases.py, at both
rule levels.  The same source, built as a stand-alone program with AddressSanitizer and UBSan, runs over the fault corpus and
must end clean with the model's answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import games_cases as GC
import games_model as GM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "games_host.cpp")
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def offsets_of(lens, stride):
    ln = np.where((lens >= 0) & (lens <= stride), lens, 0)
    return np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("games") / "libgames_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    from oracle import oracle as O
    tab = (C.c_uint8 * lib.czg_host_sizeof_tables())()
    lib.czg_host_tables(_p(np.ascontiguousarray(O.lut(), np.int16)), tab)
    srcdst = np.ascontiguousarray(O.label_srcdst(), np.uint16)

    def run(boards, side, moves, lens, results, rules, fill=0xA5):
        G, stride = moves.shape
        off = offsets_of(lens, stride)
        total = int(off[-1])
        boards = None if boards is None else np.ascontiguousarray(boards, np.uint8)
        side = None if side is None else np.ascontiguousarray(side, np.uint8)
        out = dict(records=np.full((total, 608), fill, np.uint8), valid=np.full(G, -7, np.int32), status=np.full(G, 99, np.uint8),
                   end_flags=np.full(G, 99, np.uint8), final_boards=np.full((G, 90), 99, np.uint8), final_side=np.full(G, 99, np.uint8))
        lib.czg_host_replay(tab, _p(srcdst), _p(boards), _p(side), _p(np.ascontiguousarray(moves, np.uint16)), stride,
                            _p(np.ascontiguousarray(lens, np.int32)), _p(np.ascontiguousarray(results, np.int8)), G, rules, _p(off), total,
                            _p(out["records"]), _p(out["valid"]), _p(out["status"]), _p(out["end_flags"]), _p(out["final_boards"]), _p(out["final_side"]))
        return out
    run.lib = lib
    return run


def hold(got, want):
    for k in ("valid", "status", "end_flags", "final_side", "final_boards", "records"):
        bad = np.nonzero(np.asarray(got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[0]
        assert len(bad) == 0, (k, bad[:5], got[k][bad[:2]], want[k][bad[:2]])


def test_the_opening_position_in_words(host):
    b = np.zeros(90, np.uint8)
    host.lib.czg_host_start_board(_p(b))
    assert np.array_equal(b, GM.start_board())


@pytest.mark.parametrize("rules", [0, 1])
def test_the_six_reference_games(host, rules):
    moves, lens, results, _, _ = GM.golden_games()
    hold(host(None, None, moves, lens, results, rules), GM.replay(None, None, moves, lens, results, rules))


@pytest.mark.parametrize("rules", [0, 1])
def test_the_fault_corpus(host, rules):
    c = GC.corpus()
    hold(host(c["boards"], c["side"], c["moves"], c["lens"], c["results"], rules), c["model"][rules])


def test_sanitized_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on a program with its own main, over the fault corpus at both rule levels: it must end
    clean and write the model's answer."""
    from oracle import oracle as O
    exe = str(tmp_path / "games_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGAMES_HOST_MAIN",
                           "-o", exe, SRC])
    c = GC.corpus()
    off = offsets_of(c["lens"], GC.STRIDE)
    for name, a in (("lut", np.ascontiguousarray(O.lut(), np.int16)), ("srcdst", np.ascontiguousarray(O.label_srcdst(), np.uint16)),
                    ("boards", c["boards"]), ("side", c["side"]), ("moves", c["moves"]), ("len", c["lens"]), ("result", c["results"]), ("offset", off)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    for rules in (0, 1):
        r = subprocess.run([exe, str(tmp_path), str(rules), str(GC.STRIDE)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
        raw = np.fromfile(str(tmp_path / ("out%d" % rules)), np.uint8)
        total, G, m = int(off[-1]), GC.G, c["model"][rules]
        at = total * 608
        assert np.array_equal(raw[:at].reshape(total, 608), m["records"])
        assert np.array_equal(raw[at:at + 4 * G].view(np.int32), m["valid"]); at += 4 * G
        assert np.array_equal(raw[at:at + G], m["status"]) and np.array_equal(raw[at + G:at + 2 * G], m["end_flags"]); at += 2 * G
        assert np.array_equal(raw[at:at + 90 * G].reshape(G, 90), m["final_boards"]) and np.array_equal(raw[at + 90 * G:], m["final_side"])
