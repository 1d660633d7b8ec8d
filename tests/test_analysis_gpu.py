"""cchess_zero_amd.analysis.Analyzer and the UCCI engine process on the device, with a 1-block net."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kingsafe_model as KM
import lines_cases
from cchess_zero_amd import notation

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATED = "R3k4/1R7/9/9/9/9/9/9/9/3K5 b"


@pytest.fixture(scope="module")
def analysed(rules_golden):
    """11 positions — the start as FEN, a mated one, nine of the corpus as tuples — through an Analyzer of 8 trees (two chunks,
    the second ragged), 16 playouts, 3 lines; the root statistics of every chunk are kept as the lines are read."""
    from cchess_zero_amd.analysis import Analyzer
    from cchess_zero_amd.net import PolicyValueNet

    class Tapped(Analyzer):
        def read_lines(self, allowed, n_lines, max_len):
            self.stats.append(self.engine.root_stats_host())
            return super().read_lines(allowed, n_lines, max_len)
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    safe_ones = [i for i in range(64) if not KM.kingsafe(boards[i], int(side[i]))[1] & KM.NO_SAFE_MOVE][:9]
    positions = [notation.START_FEN] + [(boards[i], int(side[i]), 0) for i in safe_ones[:4]] + [MATED] + [(boards[i], int(side[i]), 3) for i in safe_ones[4:]]
    assert len(positions) == 11
    an = Tapped(PolicyValueNet(res_block_nums=1, seed=3), 16, 8)
    an.stats = []
    return an, positions, an.analyse(positions, n_lines=3, max_len=8)


def test_analyzer_two_chunks(analysed):
    from cchess_zero_amd._lib import POS_IN_CHECK, POS_NO_SAFE_MOVE, tables
    an, positions, res = analysed
    assert len(res) == 11 and len(an.stats) == 2 and an.engine.G == 3
    label2i = tables()["label2i"]
    for i, (p, r) in enumerate(zip(positions, res)):
        board, side, _ = notation.fen_to_position(p) if isinstance(p, str) else p
        safe, flags = KM.kingsafe(board, side)
        assert r["flags"] == flags, i
        if p == MATED:
            assert r["bestmove"] is None and r["score"] is None and r["lines"] == [] and r["sims"] == 0
            assert r["flags"] & POS_NO_SAFE_MOVE and r["flags"] & POS_IN_CHECK
            continue
        assert r["sims"] == 16 and 1 <= len(r["lines"]) <= 3
        assert label2i[r["bestmove"]] in [int(l) for l in safe], i
        assert r["lines"][0]["pv"][0] == r["bestmove"] and r["score"] == r["lines"][0]["q"]
        assert all(a["visits"] >= b["visits"] for a, b in zip(r["lines"], r["lines"][1:]))
        assert all(label2i[l["pv"][0]] in [int(x) for x in safe] for l in r["lines"])
        # the score is root_stats' Q of that child, bit for bit
        st, g = an.stats[i // 8], i % 8
        at = [int(x) for x in st["label"][g, :st["count"][g]]].index(label2i[r["bestmove"]])
        assert np.float32(r["score"]).view(np.uint32) == st["Q"][g, at].view(np.uint32), i
        assert r["lines"][0]["visits"] == int(st["N"][g, at])


def test_analyzer_ban_and_capture_rules(analysed):
    from cchess_zero_amd.analysis import Analyzer
    an, positions, res = analysed
    again = an.analyse(positions[:2], n_lines=1, ban=[[res[0]["bestmove"]], None])
    assert again[0]["bestmove"] not in (None, res[0]["bestmove"]) and again[1]["bestmove"] is not None
    cap = Analyzer(an.forward.__self__, 16, 2, rules="capture")
    r = cap.analyse([MATED, notation.START_FEN])
    assert r[0]["bestmove"] is not None and r[0]["flags"] == 0 and r[0]["sims"] == 16 and r[1]["bestmove"] is not None


def test_ucci_process():
    script = "ucci\nisready\nposition startpos moves h2e2\ngo nodes 16\nquit\n"
    p = subprocess.run([sys.executable, "-m", "cchess_zero_amd.ucci", "--blocks", "1"], input=script, capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert "ucciok" in out and "readyok" in out and out[-1] == "bye"
    best = [l.split() for l in out if l.startswith("bestmove")]
    assert len(best) == 1
    from oracle import oracle as O
    board = O.apply_move(O.fen_to_board(O.START_FEN), O.labels().index("h2e2"))[0]
    assert best[0][1] in [O.labels()[int(l)] for l in KM.kingsafe(board, 1)[0]]
    info = [l.split() for l in out if l.startswith("info depth")]
    assert len(info) == 1 and info[0][info[0].index("pv") + 1] == best[0][1] and int(info[0][info[0].index("nodes") + 1]) == 16
