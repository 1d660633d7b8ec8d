"""The tablebases' build and host layers without a GPU: cz_tablebase.hip compiled to device assembly with the library's flags uses
no scratch and no more LDS than the king-safe generator, the entry points are bound and refuse a NULL context by name, the
header holds the CZ_TB_* values, the command line of cchess_zero_amd.tablebase handles its arguments and writes its JSON against
a stubbed Tablebase, and the UCCI engine's Tablebase option takes its paths against a stub searcher."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import kingsafe_model as KM
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)"
LDS = r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)"
# red to move, rook and king against the bare king: a9 mates at once (the rook on b8 holds rank 8)
WIN_FEN = "4k4/1R7/R8/9/9/9/9/9/9/3K5 w"


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__
    __graft_entry__.build_hip_only()


def _asm(tmp_path, name):
    from cchess_zero_amd import build
    assert name in build.SOURCES
    out = str(tmp_path / (name + ".s"))
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(ROOT, "cchess_zero_amd", "csrc", name)], check=True,
                   stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    return open(out).read()


def test_the_kernels_use_no_scratch_and_six_waves_fit_a_cu(tmp_path):
    text = _asm(tmp_path, "cz_tablebase.hip")
    kernels = {m.group(1): int(m.group(2)) for m in re.finditer(META, text)}
    assert len(kernels) == 3 and all(any(k in name for name in kernels) for k in ("k_tb_pass", "k_tb_probe", "k_tb_boards")), kernels
    for name, scratch in kernels.items():
        assert scratch == 0, "%s uses %d bytes of scratch" % (name, scratch)
    lds = {m.group(2): int(m.group(1)) for m in re.finditer(LDS, text)}
    ks = {m.group(2): int(m.group(1)) for m in re.finditer(LDS, _asm(tmp_path, "cz_kingsafe.hip"))}
    kingsafe = max(v for k, v in ks.items() if "k_movegen_kingsafe" in k)
    tb_pass = [v for k, v in lds.items() if "k_tb_pass" in k]
    assert len(tb_pass) == 1 and tb_pass[0] <= kingsafe and 6 * tb_pass[0] <= 160 * 1024, (lds, kingsafe)
    assert all(v <= 6 * 1024 for k, v in lds.items() if "k_tb_pass" not in k), lds


def test_the_entry_points_are_bound():
    from cchess_zero_amd import _lib
    for name, nargs in (("cz_tb_entries", 3), ("cz_tb_pass", 6), ("cz_tb_probe", 8), ("cz_tb_boards", 6)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][1]) == nargs
    L = _lib.lib()                       # a NULL context is refused before anything else is touched (no GPU needed)
    assert L.cz_tb_pass(None, b"K-K", None, None, 0, None) < 0 and b"cz_tb_pass" in L.cz_last_error()
    assert L.cz_tb_probe(None, b"K-K", None, None, None, 0, None, None) < 0 and b"cz_tb_probe" in L.cz_last_error()
    assert L.cz_tb_boards(None, b"K-K", None, 0, None, None) < 0 and b"cz_tb_boards" in L.cz_last_error()
    import ctypes as C
    n, s = C.c_longlong(), C.c_int()
    assert L.cz_tb_entries(b"KR-KAA", C.byref(n), C.byref(s)) == 0 and (n.value, s.value) == (364500, 5)
    assert L.cz_tb_entries(b"KR-KAABB", C.byref(n), C.byref(s)) == 0 and n.value == 17860500
    for bad in (b"", b"KR", b"KR-", b"RK-K", b"KRR-KRR", b"KAR-K", None):
        assert L.cz_tb_entries(bad, C.byref(n), C.byref(s)) < 0 and b"cz_tb_entries" in L.cz_last_error(), bad
    header = open(os.path.join(ROOT, "include", "cchess_hip.h")).read()
    assert re.search(r"#define CZ_TB_ILLEGAL \(-32768\)", header) and re.search(r"#define CZ_TB_UNKNOWN 32767\b", header)
    assert re.search(r"#define CZ_TB_MISS 32766\b", header) and re.search(r"#define CZ_TB_MAX_SLOTS 10\b", header)
    assert (_lib.TB_ILLEGAL, _lib.TB_UNKNOWN, _lib.TB_MISS, _lib.TB_MAX_SLOTS) == (-32768, 32767, 32766, 10)
    for name in ("cz_tb_pass", "cz_tb_probe", "cz_tb_boards"):
        assert "int %s(cz_ctx *" % name in header


# ---- the command line against a stubbed Tablebase --------------------------------------------------------------------------------
class StubTablebase:
    """Tablebase's interface as main() uses it: load, build, save, stats, tables, describe, longest"""

    def __init__(self):
        self.calls, self.tables, self.stats = [], {}, {}

    def load(self, directory, signatures=None):
        self.calls.append(("load", directory, signatures))
        if signatures is None:
            for s in ("K-K", "KR-K"):
                self.tables[s] = object()
                self.stats[s] = dict(entries=162 if s == "K-K" else 14580, legal=1, wins=2, losses=3, draws=4, longest_win=3, longest_loss=4, passes=5, seconds=0.5)
        return list(self.tables)

    def build(self, signature, progress=None):
        self.calls.append(("build", signature))
        return {"K-K": dict(entries=162, legal=108, wins=0, losses=0, draws=108, longest_win=-1, longest_loss=-1, passes=1, seconds=0.25),
                signature: dict(entries=14580, legal=8748, wins=3834, losses=4806, draws=108, longest_win=3, longest_loss=4, passes=5, seconds=0.5)}

    def save(self, directory):
        self.calls.append(("save", directory))

    def describe(self, board, side, notation="iccs", max_len=None):
        from cchess_zero_amd.notation import line_text
        self.calls.append(("describe", int(side), notation))
        if int((np.asarray(board) != 0).sum()) != 4:
            return None
        pv = [O.labels().index("a7a9")]
        text = line_text(board, side, pv, notation)
        return dict(wdl="win", plies=1, best=text[0], pv=text)

    def longest(self, signature):
        return None if signature == "K-K" else dict(fen=WIN_FEN, index=7, plies=3, pv=["a7a9"])


def test_command_line_arguments_and_json(capsys, tmp_path):
    from cchess_zero_amd import tablebase
    from cchess_zero_amd.notation import START_FEN
    d = str(tmp_path / "TB")
    stub = StubTablebase()
    rows = tablebase.main(["--build", "KR-K", "--dir", d], tb=stub)
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert out == rows and [r["signature"] for r in out] == ["K-K", "KR-K"] and stub.calls == [("build", "KR-K"), ("save", d)]
    assert list(out[1]) == ["signature", "entries", "legal", "wins", "losses", "draws", "longest_win", "longest_loss", "passes", "seconds"]
    assert out[1]["entries"] == 14580 and out[1]["longest_loss"] == 4
    # tables already in the directory are loaded, not rebuilt
    os.makedirs(d)
    open(os.path.join(d, "K-K.npz"), "w").close()
    open(os.path.join(d, "KN-K.npz"), "w").close()
    stub = StubTablebase()
    tablebase.main(["--build", "KR-K", "--dir", d], tb=stub)
    assert stub.calls[0] == ("load", d, ["K-K"]) and stub.calls[1:] == [("build", "KR-K"), ("save", d)]
    capsys.readouterr()
    # --probe: a covered and an uncovered position, the three notations
    f = tmp_path / "fens.txt"
    f.write_text(START_FEN + "\n\n")
    stub = StubTablebase()
    rows = tablebase.main(["--probe", "--fen", WIN_FEN, "--fen-file", str(f), "--dir", d], tb=stub)
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert out == rows and stub.calls == [("load", d, None), ("describe", 0, "iccs"), ("describe", 0, "iccs")]
    assert list(out[0]) == ["fen", "signature", "wdl", "plies", "best", "pv"]
    assert out[0] == dict(fen=WIN_FEN, signature="KRR-K", wdl="win", plies=1, best="a7a9", pv=["a7a9"])
    assert out[1] == dict(fen=START_FEN, signature="KRRNNCCPPPPPAABB-KRRNNCCPPPPPAABB", wdl=None, plies=None, best=None, pv=[])
    tablebase.main(["--probe", "--fen", WIN_FEN, "--dir", d, "--notation", "wxf"], tb=StubTablebase())
    assert json.loads(capsys.readouterr().out)["pv"] == ["R9+2"]
    tablebase.main(["--probe", "--fen", WIN_FEN, "--dir", d, "--notation", "chinese"], tb=StubTablebase())
    assert json.loads(capsys.readouterr().out)["best"] == "車九進二"
    # --stats and --longest
    tablebase.main(["--stats", "--dir", d], tb=StubTablebase())
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert [r["signature"] for r in out] == ["K-K", "KR-K"] and out[0]["entries"] == 162 and out[1]["passes"] == 5
    tablebase.main(["--longest", "--dir", d], tb=StubTablebase())
    out = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert out == [dict(signature="K-K", fen=None, index=None, plies=None, pv=[]), dict(signature="KR-K", fen=WIN_FEN, index=7, plies=3, pv=["a7a9"])]
    # bad signatures, bad FENs, missing and contradictory arguments exit
    for bad in (["--build", "KR", "--dir", d], ["--build", "RK-K", "--dir", d], ["--build", "KRRR-K", "--dir", d], ["--build", "KAR-K", "--dir", d],
                ["--build", "KR-K"], ["--probe", "--dir", d], ["--probe", "--fen", "not a fen", "--dir", d], ["--stats", "--fen", WIN_FEN, "--dir", d],
                ["--dir", d], ["--build", "KR-K", "--stats", "--dir", d], ["--probe", "--fen", WIN_FEN, "--dir", d, "--notation", "pgn"]):
        with pytest.raises(SystemExit):
            tablebase.main(bad, tb=StubTablebase())
        capsys.readouterr()


def test_host_helpers():
    from cchess_zero_amd import tablebase as T
    assert T.sub_signature("KR-KAA", 1) == "K-KAA" and T.sub_signature("KR-KAA", 4) == "KR-KA"
    assert T.closure_names("KR-KAA") == {"K-K", "K-KA", "K-KAA", "KR-K", "KR-KA", "KR-KAA"}
    assert T.closure("KP-KP") == ["K-K", "K-KP", "KP-K", "KP-KP"] and T.entries("KP-KP") == (490050, 4)
    with pytest.raises(ValueError):
        T.entries("KPK")
    counts = np.bincount(O.fen_to_board(O.START_FEN), minlength=15)
    assert T.signature_of_counts(counts) == "KRRNNCCPPPPPAABB-KRRNNCCPPPPPAABB"
    counts[8] = 0
    assert T.signature_of_counts(counts) is None
    assert T.wdl_of(0) == ("draw", None) and T.wdl_of(38) == ("win", 37) and T.wdl_of(-1) == ("loss", 0) and T.wdl_of(-21) == ("loss", 20)
    assert T.wdl_of(T.TB_MISS) == (None, None) and T.wdl_of(T.TB_ILLEGAL) == (None, None)


# ---- UCCI Tablebase against a stub searcher ------------------------------------------------------------------------------------------
class StubSearcher:
    """The searcher interface of UcciEngine with a scripted search: one line, the first allowed king-safe move; tablebase() is
    counted and answers what the test scripted."""
    width = 1

    def __init__(self, found):
        self.found, self.tb_calls, self.searches = found, [], 0

    def set_position(self, board, side, rr):
        self.pos = (np.array(board, np.uint8), int(side))

    def kingsafe_mask(self):
        safe, flags = KM.kingsafe(*self.pos)
        return KM.mask_of(safe), int(flags)

    def tablebase(self, directory):
        self.tb_calls.append(directory)
        return self.found

    def search(self, playouts):
        self.searches += 1
        return playouts

    def lines(self, allowed, n_lines, max_len):
        first = next(int(l) for l in KM.kingsafe(*self.pos)[0] if (int(allowed[int(l) >> 5]) >> (int(l) & 31)) & 1)
        return [dict(pv=[first], visits=[5], q=[0.25])]


def _session(script, searcher):
    from cchess_zero_amd.ucci import UcciEngine
    out = io.StringIO()
    ticks = iter(range(1000))
    UcciEngine(searcher, io.StringIO(script), out, clock=lambda: next(ticks) * 0.001).run()
    return out.getvalue().splitlines()


def test_ucci_tablebase_control_flow():
    L = O.labels()
    a7a9, e9e8, b8b9 = L.index("a7a9"), L.index("e9e8"), L.index("b8b9")
    pos = "position fen %s\n" % WIN_FEN
    # a covered win: the info line of the table and bestmove, no search
    s = StubSearcher((2, [a7a9]))
    lines = _session("setoption Tablebase /some/dir with spaces\n" + pos + "go nodes 16\nquit\n", s)
    info = [l for l in lines if l.startswith("info depth")]
    assert s.tb_calls == ["/some/dir with spaces"] and s.searches == 0
    assert len(info) == 1 and re.fullmatch(r"info depth 1 score 29999 nodes 0 time \d+ pv a7a9", info[0]), info
    assert lines[-2:] == ["bestmove a7a9", "bye"]
    # a longer win, in another notation: the score follows the plies, the second move is the ponder move
    s = StubSearcher((4, [a7a9, e9e8, b8b9]))
    lines = _session("setoption Tablebase TB\nsetoption Notation wxf\n" + pos + "go\nquit\n", s)
    assert [l for l in lines if l.startswith("info depth")][0].startswith("info depth 3 score 29997 nodes 0 ") and lines[-2] == "bestmove a7a9 ponder e9e8"
    assert " pv R9+2 " in [l for l in lines if l.startswith("info depth")][0]
    # a covered loss and a covered draw
    s = StubSearcher((-5, [a7a9, e9e8]))
    lines = _session("setoption Tablebase TB\n" + pos + "go\nquit\n", s)
    assert [l for l in lines if l.startswith("info depth")][0].startswith("info depth 2 score -29996 nodes 0 ") and s.searches == 0
    s = StubSearcher((0, [a7a9]))
    lines = _session("setoption Tablebase TB\n" + pos + "go\nquit\n", s)
    assert [l for l in lines if l.startswith("info depth")][0].startswith("info depth 1 score 0 nodes 0 ") and lines[-2] == "bestmove a7a9" and s.searches == 0
    # the table's best move is banned: the search runs as without the option
    s = StubSearcher((2, [a7a9]))
    lines = _session("setoption Tablebase TB\n" + pos + "banmoves a7a9\ngo nodes 16\nquit\n", s)
    assert s.tb_calls == ["TB"] and s.searches >= 1
    best = [l for l in lines if l.startswith("bestmove")]
    assert len(best) == 1 and best[0] != "bestmove a7a9" and not any("score 29999" in l for l in lines)
    # a position no table covers: the search runs
    s = StubSearcher(None)
    lines = _session("setoption Tablebase TB\n" + pos + "go nodes 16\nquit\n", s)
    assert s.tb_calls == ["TB"] and s.searches >= 1 and any(l.startswith("bestmove") for l in lines)
    # the option unset (the default, and after setoption Tablebase none): the tables are never asked
    for script in (pos + "go nodes 16\nquit\n", "setoption Tablebase TB\nsetoption Tablebase none\n" + pos + "go nodes 16\nquit\n"):
        s = StubSearcher((2, [a7a9]))
        lines = _session(script, s)
        assert s.tb_calls == [] and s.searches >= 1 and any(l.startswith("bestmove") for l in lines)
    # a searcher without the method (the interface of earlier versions) is only asked once the option is set
    class Old(StubSearcher):
        tablebase = None
    s = Old(None)
    lines = _session(pos + "go nodes 16\nquit\n", s)
    assert s.searches >= 1 and any(l.startswith("bestmove") for l in lines)
