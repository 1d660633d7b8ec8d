"""cz_notation.h (the token decode cz_games_read runs inside the replay: one lane = one game) compiled for the HOST and held, on
the CPU, to tests/notation_model.py byte for byte over the corpus of tests/notation_cases.py at both rule levels: records, valid,
status, end_flags, final boards and sides, labels_out.  The same source, built as a stand-alone program with AddressSanitizer
and UBSan, runs over the corpus and must end clean with the model's answer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import notation_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "notation_host.cpp")
KEYS = ("valid", "status", "end_flags", "final_side", "final_boards", "labels_out", "records")
_p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)


def offsets_of(lens, stride):
    ln = np.where((lens >= 0) & (lens <= stride), lens, 0)
    return np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("notation") / "libnotation_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    from oracle import oracle as O
    tab = (C.c_uint8 * lib.czn_host_sizeof_tables())()
    lib.czn_host_tables(_p(np.ascontiguousarray(O.lut(), np.int16)), tab)
    srcdst = np.ascontiguousarray(O.label_srcdst(), np.uint16)

    def run(boards, side, tokens, lens, results, rules, fill=0xA5):
        G, stride = tokens.shape
        off = offsets_of(lens, stride)
        total = int(off[-1])
        out = dict(records=np.full((total, 608), fill, np.uint8), valid=np.full(G, -7, np.int32), status=np.full(G, 99, np.uint8),
                   end_flags=np.full(G, 99, np.uint8), final_boards=np.full((G, 90), 99, np.uint8), final_side=np.full(G, 99, np.uint8),
                   labels_out=np.full((G, stride), 0x5A5A, np.uint16))
        lib.czn_host_read(tab, _p(srcdst), _p(np.ascontiguousarray(boards, np.uint8)), _p(np.ascontiguousarray(side, np.uint8)),
                          _p(np.ascontiguousarray(tokens, np.uint32)), stride, _p(np.ascontiguousarray(lens, np.int32)),
                          _p(np.ascontiguousarray(results, np.int8)), G, rules, _p(off), total, _p(out["records"]), _p(out["valid"]), _p(out["status"]),
                          _p(out["end_flags"]), _p(out["final_boards"]), _p(out["final_side"]), _p(out["labels_out"]))
        return out
    run.lib = lib
    return run


def hold(got, want):
    for k in KEYS:
        bad = np.nonzero(np.asarray(got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[0]
        assert len(bad) == 0, (k, bad[:5], got[k][bad[:2]], want[k][bad[:2]])


@pytest.mark.parametrize("rules", [0, 1])
def test_the_corpus(host, rules):
    c = NC.corpus()
    hold(host(c["boards"], c["side"], c["tokens"], c["lens"], c["results"], rules), c["model"][rules])


def test_label_tokens_alone_are_the_label_replay(host):
    """the fault corpus of cz_games_replay as small tokens: games_model's answer, and the labels of the plies made"""
    import games_cases as GC
    c = GC.corpus()
    for rules in (0, 1):
        got = host(c["boards"], c["side"], c["moves"].astype(np.uint32), c["lens"], c["results"], rules)
        want = dict(c["model"][rules])
        want["labels_out"] = np.where(np.arange(GC.STRIDE)[None, :] < want["valid"][:, None], c["moves"], 0xFFFF).astype(np.uint16)
        hold(got, want)


def test_sanitized_stand_alone_program(tmp_path):
    """-fsanitize=address,undefined on a program with its own main, over the corpus at both rule levels: it must end clean and
    write the model's answer."""
    from oracle import oracle as O
    exe = str(tmp_path / "notation_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DNOTATION_HOST_MAIN",
                           "-o", exe, SRC])
    c = NC.corpus()
    stride = c["stride"]
    off = offsets_of(c["lens"], stride)
    for name, a in (("lut", np.ascontiguousarray(O.lut(), np.int16)), ("srcdst", np.ascontiguousarray(O.label_srcdst(), np.uint16)),
                    ("boards", c["boards"]), ("side", c["side"]), ("tokens", c["tokens"]), ("len", c["lens"]), ("result", c["results"]), ("offset", off)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    for rules in (0, 1):
        r = subprocess.run([exe, str(tmp_path), str(rules), str(stride)], capture_output=True, text=True)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
        raw = np.fromfile(str(tmp_path / ("out%d" % rules)), np.uint8)
        total, G, m = int(off[-1]), NC.G, c["model"][rules]
        at = total * 608
        assert np.array_equal(raw[:at].reshape(total, 608), m["records"])
        assert np.array_equal(raw[at:at + 4 * G].view(np.int32), m["valid"]); at += 4 * G
        assert np.array_equal(raw[at:at + G], m["status"]) and np.array_equal(raw[at + G:at + 2 * G], m["end_flags"]); at += 2 * G
        assert np.array_equal(raw[at:at + 90 * G].reshape(G, 90), m["final_boards"]) and np.array_equal(raw[at + 90 * G:at + 91 * G], m["final_side"])
        assert np.array_equal(raw[at + 91 * G:].view(np.uint16).reshape(G, stride), m["labels_out"])
