"""The table set without a GPU: the material key and the directory of cchess_zero_amd/csrc/cz_tablebase.h compiled for the host
(tests/tablebase_set_host.cpp, plain and under -fsanitize=address,undefined, run as that program) against the key
Tablebase.signatures_of defines; tests/tablebase_set_model.py's mixed probe and adjudication verdict on the recorded tables;
k_tb_probe_set's resources from its device assembly; the bindings, the header and the host layer's options."""
import os
import re
import subprocess

import numpy as np
import pytest

import tablebase_model as TM
import tablebase_set_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tablebase_set_host.cpp")
FIXTURE = ("KP-KP", "KR-KAA", "KN-KA", "KN-KB", "KR-K", "KC-K")   # the tables tests/test_hip_tablebase.py builds, with their closures


def fixture_signatures():
    out = []
    for s in FIXTURE:
        out += [c for c in TM.closure(s) if c not in out]
    return out


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tbset") / ("tablebase_set_host_" + request.param))
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", out, SRC])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    return r


def boards_of(sig, n, rng):
    """n boards of a signature whose slots do not overlap"""
    out = []
    while len(out) < n:
        b, _ = TM.unrank(sig, int(rng.integers(TM.entries(sig))))
        if b is not None:
            out.append(b)
    return out


def python_key(boards):
    """Tablebase.signatures_of's key, with its own expressions, in numpy"""
    boards = np.asarray(boards, np.uint8).reshape(-1, 90)
    key = (boards > 14).any(1).astype(np.int64) << 45
    for c in range(1, 15):
        key += np.minimum((boards == c).sum(1), 7).astype(np.int64) << (3 * c)
    return key


def test_the_key_is_signatures_ofs(exe, tmp_path):
    from cchess_zero_amd.rules import START_BOARD
    rng = np.random.default_rng(5)
    sigs = fixture_signatures()
    boards, owner = [], []
    for s in sigs:
        b = boards_of(s, 6, rng)
        boards += b
        owner += [s] * len(b)
    start = np.asarray(START_BOARD, np.uint8).reshape(90)
    foreign = []
    for byte, at in ((15, 40), (16, 41), (0x11, 0), (200, 89), (255, 44)):   # above 14: alone, and where its low nibble reads as a piece code
        b = boards_of("KR-KAA", 1, rng)[0].copy()
        at = at if b[at] == 0 else int(np.nonzero(b == 0)[0][0])
        b[at] = byte
        foreign.append(b)
    many = start.copy()
    many[27:63] = 0                      # 22 pieces: no pawns
    eight = np.zeros(90, np.uint8)
    eight[[3, 86]] = (1, 8)
    eight[45:53] = 6                     # eight red pawns: a count above 7 reads 7
    extra = [start, many, eight, np.zeros(90, np.uint8)] + foreign
    all_boards = np.stack(boards + extra)
    path = tmp_path / "boards.bin"
    all_boards.tofile(str(path))
    r = run(exe, "keys", path)
    assert r.returncode == 0, r.stderr
    got = np.array([int(x) for x in r.stdout.split()], np.int64)
    want = python_key(all_boards)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    assert all(SM.material_key(b) == int(k) for b, k in zip(all_boards, want))
    assert all(int(k) >> 45 == 1 for k in want[-len(foreign):]) and not (want[:-len(foreign)] >> 45).any()
    # the key of a descriptor is the key of any board of its signature, and of no other signature's
    d = run(exe, "desc", *sigs)
    dkeys = [int(x) for x in d.stdout.split()]
    assert len(dkeys) == len(sigs) == len(set(dkeys))
    by_sig = dict(zip(sigs, dkeys))
    assert all(by_sig[s] == int(k) for s, k in zip(owner, want)) and all(by_sig[s] == SM.signature_key(s) for s in sigs)
    two = run(exe, "desc", "KP-K", "K-KP", "KR-KAABB", "RK-K").stdout.split("\n")
    assert two[0] != two[1] and int(two[0]) == (1 << 3) + (1 << 18) + (1 << 24) and int(two[1]) == (1 << 3) + (1 << 24) + (1 << 39)
    assert int(two[2]) == SM.signature_key("KR-KAABB") and two[3].startswith("bad ")


def test_the_directory(exe):
    sigs = fixture_signatures()
    want = sorted(sigs, key=SM.signature_key)
    rng = np.random.default_rng(9)
    for trial in range(4):
        given = list(sigs) if trial == 0 else list(reversed(sigs)) if trial == 1 else [sigs[i] for i in rng.permutation(len(sigs))]
        r = run(exe, "dir", *given)
        lines = r.stdout.strip().split("\n")
        assert r.returncode == 0 and lines[0].split() == want and lines[-1] == "0 wrong", r.stdout
        assert [l.split(" at ") for l in lines[1:-1]] == [[s, str(want.index(s))] for s in given]
    one = run(exe, "dir", "KR-K").stdout.split("\n")
    assert one[0] == "KR-K" and one[1] == "KR-K at 0" and one[2] == "0 wrong"
    assert run(exe, "dir").stdout.strip() == "refused n"
    assert run(exe, "dir", "KR-K", "KN-K", "KR-K").stdout.strip() == "refused twice KR-K"
    assert run(exe, "dir", "KR-K", "KRK").stdout.strip() == "refused bad KRK"
    assert run(exe, "dir", "KR-K", "KAR-K").stdout.strip() == "refused bad KAR-K"
    sides = ("K", "KR", "KP", "KA", "KB", "KAA", "KBB", "KAB", "KAAB", "KABB", "KAABB", "KPA", "KPB", "KPAA", "KPBB", "KPAB")   # all below 2^31 entries
    full = [a + "-" + b for a in sides for b in sides]
    assert len(full) == 256 and run(exe, "dir", *full).stdout.strip().endswith("0 wrong")   # a full directory: every place is found
    assert run(exe, "dir", *(full + ["KRA-K"])).stdout.strip() == "refused n"


def test_the_model_probes_a_mixed_batch_on_the_recorded_tables():
    values, _ = TM.golden()
    order = ["KR-K", "K-K", "KN-KA", "KP-K", "KR-KAA"]
    rng = np.random.default_rng(2)
    seen = set()
    for s in order + ["KN-K"]:
        for i in rng.integers(TM.entries(s), size=40):
            b, side = TM.unrank(s, int(i))
            if b is None:
                assert SM.probe(values, order, np.zeros(90, np.uint8), side) == (SM.MISS, -1)
                continue
            v, w = SM.probe(values, order, b, side)
            if s not in order:
                assert (v, w) == (SM.MISS, -1)
            else:
                assert w == order.index(s) and v == int(values[s][TM.rank(s, b, side)])
                seen.add("illegal" if v == SM.ILLEGAL else "win" if v > 0 else "loss" if v < 0 else "draw")
    assert seen == {"illegal", "win", "loss", "draw"}
    b = np.zeros(90, np.uint8)
    b[[4, 10, 85, 66, 68]] = (1, 3, 8, 9, 9)
    assert SM.probe(values, order, b, 0) == (int(values["KR-KAA"][TM.rank("KR-KAA", b, 0)]), order.index("KR-KAA"))
    outside = b.copy()
    outside[68], outside[67] = 0, 9      # a black advisor on a square no advisor reaches
    assert SM.probe(values, order, outside, 0) == (SM.ILLEGAL, order.index("KR-KAA"))
    foreign = b.copy()
    foreign[0 if b[0] == 0 else 1] = 15
    assert SM.probe(values, order, foreign, 0) == (SM.MISS, -1)


def test_the_model_places_the_table_among_the_endings():
    V = SM.verdict
    assert V(4, 0) == (SM.TABLEBASE, 1) and V(4, 1) == (SM.TABLEBASE, 0)        # the side to move wins
    assert V(-3, 0) == (SM.TABLEBASE, 0) and V(-1, 1) == (SM.TABLEBASE, 1)      # the side to move loses
    assert V(0, 0) == V(0, 1) == (SM.TABLEBASE, -1)
    assert V(SM.MISS, 0) == V(SM.ILLEGAL, 1) == (0, -1)
    # behind what the choose found on the root that was not left
    assert V(4, 0, rep=SM.REP_DRAW) == (SM.REPETITION, -1) and V(4, 0, rep=SM.REP_RED_LOSES) == (SM.PERPETUAL, 0)
    assert V(4, 0, rep=SM.REP_BLACK_LOSES, by_chase=True) == (SM.CHASE, 1)
    assert V(4, 0, mated=True) == (SM.MATE, 0) and V(-2, 1, resigned=True) == (SM.RESIGN, 1) and V(4, 0, aborted=True) == (SM.ABORTED, -1)
    # in front of check_end and the ply cap: a forced mate is a mate whatever the no-capture counter says
    assert V(4, 0, rr=60) == (SM.TABLEBASE, 1) and V(0, 1, ply=9, max_plies=9) == (SM.TABLEBASE, -1) and V(-2, 0, black_king=False) == (SM.TABLEBASE, 0)
    assert V(SM.MISS, 0, rr=60) == (SM.RR60, -1) and V(SM.MISS, 0, ply=9, max_plies=9) == (SM.PLY_CAP, -1)
    assert V(SM.MISS, 1, red_king=False) == (SM.KING, 0) and V(SM.ILLEGAL, 0, black_king=False) == (SM.KING, 1)
    assert [SM.result_for_a(l, a) for l, a in ((0, 1), (0, 0), (1, 1), (1, 0), (-1, 1))] == [-1, 1, 1, -1, 0]


# ---- the library side, without a GPU ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def library():
    import __graft_entry__
    __graft_entry__.build_hip_only()
    from cchess_zero_amd import _lib
    return _lib


def test_the_kernel_uses_no_scratch_no_barrier_and_little_lds(library, tmp_path):
    from cchess_zero_amd import build
    assert "cz_tablebase_set.hip" in build.SOURCES
    out = str(tmp_path / "cz_tablebase_set.s")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(ROOT, "cchess_zero_amd", "csrc", "cz_tablebase_set.hip")],
                   check=True, stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    text = open(out).read()
    meta = {m.group(2): (int(m.group(1)), int(m.group(3))) for m in
            re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", text)}
    assert len(meta) == 2 and all("k_tb_probe_set" in k for k in meta), meta   # boards 90 bytes apart, and rows read in place
    for name, (lds, scratch) in meta.items():
        assert scratch == 0, "%s uses %d bytes of scratch" % (name, scratch)
        assert lds <= 8 * 1024, (name, lds)                                      # sixteen waves per CU keep their boards and keys
    assert "s_barrier" not in text                                               # CZF_WAVE_FENCE only
    assert len(re.findall(r"s_load_dwordx16", text)) >= 2                        # the waterfall's entry comes through scalar loads


def test_the_entry_points_are_bound(library):
    import ctypes as C
    _lib = library
    for name, nargs in (("cz_tb_set_create", 5), ("cz_tb_set_destroy", 1), ("cz_tb_set_probe", 7), ("cz_selfplay_set_tablebase", 2),
                        ("cz_selfplay_tablebase_stats", 2), ("cz_match_set_tablebase", 2)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][1]) == nargs
    L = _lib.lib()
    h = C.c_void_p()
    assert L.cz_tb_set_create(None, 1, None, None, C.byref(h)) < 0 and b"cz_tb_set_create" in L.cz_last_error() and not h.value
    assert L.cz_tb_set_probe(None, None, None, None, 0, None, None) < 0 and b"cz_tb_set_probe" in L.cz_last_error()
    assert L.cz_selfplay_set_tablebase(None, None) < 0 and b"cz_selfplay_set_tablebase" in L.cz_last_error()
    assert L.cz_selfplay_tablebase_stats(None, None) < 0 and b"cz_selfplay_tablebase_stats" in L.cz_last_error()
    assert L.cz_match_set_tablebase(None, None) < 0 and b"cz_match_set_tablebase" in L.cz_last_error()
    assert L.cz_tb_set_destroy(None) == 0
    header = open(os.path.join(ROOT, "include", "cchess_hip.h")).read()
    assert re.search(r"#define CZ_MATCH_TABLEBASE 11\b", header) and re.search(r"#define CZ_TB_SET_MAX 256\b", header)
    assert (_lib.MATCH_TABLEBASE, _lib.TB_SET_MAX, _lib.SP_TABLEBASE_STATS) == (11, 256, ("tablebase",)) == (SM.TABLEBASE, 256, ("tablebase",))


def test_the_host_layer_counts_and_refuses(library):
    from cchess_zero_amd import arena, selfplay
    assert arena.REASONS[11] == "tablebase"
    reason = [1, 11, 4, 10, 11]
    assert arena.is_scored(reason).tolist() == [True, False, False, False, False]
    assert arena.is_scored(reason, tablebase=True).tolist() == [True, True, False, False, True]
    assert arena.is_scored(reason, resign=True, tablebase=True).tolist() == [True, True, False, True, True]
    r = arena.MatchResult([1, -1, 0, 1], [1, 0, 1, 0], [9, 9, 9, 9], [11, 11, 11, 1], None, 10, 1.0, [], rules="xiangqi", tablebase=True)
    d = r.to_dict()
    assert (r.tablebases, r.scored, r.wins, r.draws, r.losses) == (3, 4, 2, 1, 1) and d["tablebase"] is True and d["tablebases"] == 3 == d["reasons"]["tablebase"]
    plain = arena.MatchResult([1, -1], [1, 0], [9, 9], [1, 1], None, 10, 1.0, [])
    assert plain.tablebase is False and plain.tablebases == 0 and plain.to_dict()["tablebases"] == 0
    with pytest.raises(ValueError, match="tablebase needs rules='xiangqi'"):
        arena.Match((lambda p: None, 1), (lambda p: None, 1), ["x"], slots=2, tablebase=object())
    with pytest.raises(ValueError, match="tablebase needs rules='xiangqi'"):
        selfplay.SelfPlay(None, None, 1, tablebase=object())
    with pytest.raises(SystemExit):
        arena.main(["--tablebase", ROOT])          # without --rules xiangqi
    with pytest.raises(SystemExit):
        arena.main(["--rules", "xiangqi", "--tablebase", os.path.join(ROOT, "no-such-directory")])
