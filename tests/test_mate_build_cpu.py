"""The mate search's build and host layers without a GPU: the new kernels compiled to device assembly with the library's flags
use no scratch (and keep the LDS of the king-safe kernels they share a wave with), the entry points are bound, the command
line of cchess_zero_amd.mate handles its arguments and writes its JSON against a stubbed Rules, and the UCCI engine's MateSearch
option takes the three paths: mate found, first move banned, option off."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import kingsafe_model as KM
from cchess_zero_amd.notation import START_FEN
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META = r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)"
# red to move mates in one: the rook goes to the back rank, the other rook holds rank 8, the red king file d
MATE_IN_1 = "4k4/1R7/R8/9/9/9/9/9/9/3K5 w"


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


def test_the_new_kernels_use_no_scratch(tmp_path):
    text = _asm(tmp_path, "cz_kingsafe.hip")
    kernels = [(m.group(1), int(m.group(2))) for m in re.finditer(META, text)]
    checks = [k for k in kernels if "k_movegen_checks" in k[0]]
    assert len(checks) == 2 and len([k for k in kernels if "k_movegen_kingsafe" in k[0]]) == 4, kernels      # list / count forms; the four old ones
    for name, scratch in kernels:
        assert scratch == 0, "%s uses %d bytes of scratch" % (name, scratch)
    lds = {m.group(2): int(m.group(1)) for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)", text)}
    old = max(v for k, v in lds.items() if "k_movegen_kingsafe" in k)
    assert all(v <= old for k, v in lds.items() if "k_movegen_checks" in k), lds                               # six waves per CU, as before
    text = _asm(tmp_path, "cz_mate.hip")
    kernels = [(m.group(1), int(m.group(2))) for m in re.finditer(META, text)]
    assert len(kernels) == 1 and "k_mate_backup" in kernels[0][0] and kernels[0][1] == 0, kernels


def test_the_entry_points_are_bound():
    from cchess_zero_amd import _lib
    assert "cz_movegen_checks" in _lib.EXPORTS and len(_lib._SIGS["cz_movegen_checks"][1]) == 8
    assert "cz_mate_backup" in _lib.EXPORTS and len(_lib._SIGS["cz_mate_backup"][1]) == 11
    L = _lib.lib()                       # a NULL context is refused before anything else is touched (no GPU needed)
    assert L.cz_movegen_checks(None, None, None, 0, None, None, None, 0) < 0 and b"cz_movegen_checks" in L.cz_last_error()
    assert L.cz_mate_backup(None, None, 0, 0, None, None, None, 0, 0, None, None) < 0 and b"cz_mate_backup" in L.cz_last_error()
    header = open(os.path.join(ROOT, "include", "cchess_hip.h")).read()
    assert re.search(r"#define CZ_MATE_NONE 0x7FFF\b", header) and _lib.MATE_NONE == 0x7FFF
    assert "int cz_movegen_checks(cz_ctx *" in header and "int cz_mate_backup(cz_ctx *" in header


# ---- the command line against a stubbed Rules ----------------------------------------------------------------------------------
class StubRules:
    """Rules.mate's interface: answers every position with a mate in one by its first checking move that mates (the model's)."""

    def __init__(self):
        self.calls = []

    def mate(self, boards, side, plies, attacker="checks", chunk=None, node_limit=None):
        import mate_model as MM
        self.calls.append(dict(n=len(boards), plies=plies, attacker=attacker, node_limit=node_limit))
        st, d, pv = MM.solve_batch(boards, side, 1, attacker)
        wide = np.full((len(boards), plies), 0xFFFF, np.uint16)
        wide[:, :1] = pv
        if node_limit is not None:
            st = np.where(st == 2, 2, 3).astype(np.uint8)
        return dict(status=st, dist=d, pv=wide, nodes=np.full(len(boards), 7, np.int64))


def test_command_line_arguments_and_json(capsys, tmp_path):
    from cchess_zero_amd import mate
    stub = StubRules()
    f = tmp_path / "fens.txt"
    f.write_text(START_FEN + "\n\n")
    res = mate.main(["--fen", MATE_IN_1, "--fen-file", str(f), "--plies", "5"], rules=stub)
    rows = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert stub.calls == [dict(n=2, plies=5, attacker="checks", node_limit=None)] and len(rows) == 2 and rows == res
    assert list(rows[0]) == ["fen", "status", "mate_in", "plies", "pv", "nodes", "seconds"]
    assert rows[0]["fen"] == MATE_IN_1 and rows[0]["status"] == "mate" and rows[0]["mate_in"] == 1 and rows[0]["plies"] == 1
    assert rows[0]["pv"] == ["a7a9"] and rows[0]["nodes"] == 7 and rows[0]["seconds"] >= 0
    assert rows[1]["fen"] == START_FEN and rows[1]["status"] == "none" and rows[1]["mate_in"] is None and rows[1]["plies"] is None and rows[1]["pv"] == []
    # the options reach the solver; the notation is applied to the line
    mate.main(["--fen", MATE_IN_1, "--all-moves", "--node-limit", "1000", "--notation", "wxf"], rules=stub)
    row = json.loads(capsys.readouterr().out)
    assert stub.calls[-1] == dict(n=1, plies=9, attacker="all", node_limit=1000) and row["status"] == "node_limit" and row["pv"] == []
    mate.main(["--fen", MATE_IN_1, "--plies", "1", "--notation", "wxf"], rules=stub)
    assert json.loads(capsys.readouterr().out)["pv"] == ["R9+2"]
    mate.main(["--fen", MATE_IN_1, "--plies", "1", "--notation", "chinese"], rules=stub)
    assert json.loads(capsys.readouterr().out)["pv"] == ["車九進二"]
    # the kings face each other on file d, red to move: the mover can take the king, a bad root
    mate.main(["--fen", "3k5/1R7/R8/9/9/9/9/9/9/3K5 w", "--plies", "3"], rules=stub)
    assert json.loads(capsys.readouterr().out)["status"] == "bad_root"
    for bad in (["--plies", "4", "--fen", MATE_IN_1], ["--plies", "17", "--fen", MATE_IN_1], [], ["--fen", "not a fen"], ["--fen", MATE_IN_1, "--node-limit", "0"]):
        with pytest.raises(SystemExit):
            mate.main(bad, rules=stub)
        capsys.readouterr()


# ---- UCCI MateSearch against a stub solver -----------------------------------------------------------------------------------------
class StubSearcher:
    """The searcher interface of UcciEngine with a scripted search: one line, the first king-safe move; mate() is counted."""
    width = 1

    def __init__(self, found):
        self.found, self.mate_calls, self.searches = found, [], 0

    def set_position(self, board, side, rr):
        self.pos = (np.array(board, np.uint8), int(side))

    def kingsafe_mask(self):
        safe, flags = KM.kingsafe(*self.pos)
        return KM.mask_of(safe), int(flags)

    def mate(self, plies):
        self.mate_calls.append(plies)
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


def test_ucci_mate_search_control_flow():
    L = O.labels()
    a7a9, b8b9 = L.index("a7a9"), L.index("b8b9")
    pos = "position fen %s\n" % MATE_IN_1
    # mate found: the info line of the mate and bestmove, no search
    s = StubSearcher((1, [a7a9], 12))
    lines = _session("setoption MateSearch 5\n" + pos + "go nodes 16\nquit\n", s)
    info = [l for l in lines if l.startswith("info depth")]
    assert s.mate_calls == [5] and s.searches == 0
    assert len(info) == 1 and re.fullmatch(r"info depth 1 score 29999 nodes 12 time \d+ pv a7a9", info[0]), info
    assert lines[-2:] == ["bestmove a7a9", "bye"]
    # a longer line: depth and score follow the distance, the second move is the ponder move
    s = StubSearcher((3, [a7a9, L.index("d9e9"), b8b9], 40))
    lines = _session("setoption MateSearch 3\n" + pos + "go\nquit\n", s)
    assert [l for l in lines if l.startswith("info depth")][0].startswith("info depth 3 score 29997 nodes 40 ") and lines[-2] == "bestmove a7a9 ponder d9e9"
    # the mate's first move is banned: the search runs as without the option
    s = StubSearcher((1, [a7a9], 12))
    lines = _session("setoption MateSearch 5\n" + pos + "banmoves a7a9\ngo nodes 16\nquit\n", s)
    assert s.mate_calls == [5] and s.searches >= 1
    best = [l for l in lines if l.startswith("bestmove")]
    assert len(best) == 1 and best[0] != "bestmove a7a9" and not any("score 29999" in l for l in lines)
    # no mate: the search runs
    s = StubSearcher(None)
    lines = _session("setoption MateSearch 5\n" + pos + "go nodes 16\nquit\n", s)
    assert s.mate_calls == [5] and s.searches >= 1 and any(l.startswith("bestmove") for l in lines)
    # the option off (the default, and after setoption MateSearch 0): the solver is never called
    for script in (pos + "go nodes 16\nquit\n", "setoption MateSearch 5\nsetoption MateSearch 0\n" + pos + "go nodes 16\nquit\n"):
        s = StubSearcher((1, [a7a9], 12))
        lines = _session(script, s)
        assert s.mate_calls == [] and s.searches >= 1 and any(l.startswith("bestmove") for l in lines)
    # an even or oversized horizon is refused with an info string and leaves the option as it was
    s = StubSearcher((1, [a7a9], 12))
    lines = _session("setoption MateSearch 4\nsetoption MateSearch 17\n" + pos + "go nodes 16\nquit\n", s)
    assert sum(l.startswith("info string setoption MateSearch") for l in lines) == 2 and s.mate_calls == []
