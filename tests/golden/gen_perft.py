"""Writes tests/golden/perft.json: perft tables under Xiangqi rules, computed on the CPU by tests/perft_host.cpp (a recursive
perft over cz_kingsafe.h, the library's king-safe generator compiled for the host).  No GPU code is involved.

    python tests/golden/gen_perft.py            (a few minutes: the start position to depth 5 with all four columns)

The start position's node row is the published Xiangqi perft table; the generator asserts that it reproduces it, and the other
three columns as first computed with it.  Depth 6 (5 392 831 844, published; five minutes on one core with the last ply
counted) is recomputed only with --depth6 and written as the published number otherwise.  The other positions come from
tests/golden/rules.npz and conftest.open_boards; the conditions on the corpus are asserted, so that it cannot quietly become
trivial."""
import json
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import kingsafe_model as M   # noqa: E402
import perft_host            # noqa: E402
import perft_model           # noqa: E402
from conftest import open_boards   # noqa: E402
from oracle import oracle as O     # noqa: E402

START = {"nodes": [1, 44, 1920, 79666, 3290240, 133312995], "captures": [0, 2, 72, 3159, 115365, 4917734],
         "checks": [0, 0, 6, 384, 19380, 953251], "mates": [0, 0, 0, 0, 0, 584]}
START_DEPTH6 = 5392831844


def split_perft(host, board, side, depth, stats=True):
    """host(board, side, depth) as the root's row plus the sum of its children's, the children on a thread each"""
    root = host(board, side, 1, stats)
    moves, _ = M.kingsafe(board, side)
    kids = [perft_model.make_move(board, m) for m in moves]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        rows = list(ex.map(lambda k: host(k[0], 1 - side, depth - 1, stats), kids))
    out = {}
    for name in root:
        col = np.zeros(depth + 1, np.int64)
        col[:2] = root[name][:2]
        for (_, taken), r in zip(kids, rows):
            col[2:] += r[name][1:]
        out[name] = col
    return out


def kings_between(board):
    """the pieces between the two kings when they share a file (the flying general acts at 0, pins at 1), else None"""
    k, K = np.nonzero(board == 8)[0], np.nonzero(board == 1)[0]
    if len(k) != 1 or len(K) != 1 or k[0] % 9 != K[0] % 9:
        return None
    lo, hi = sorted((int(k[0]), int(K[0])))
    return int((board[lo + 9:hi:9] != 0).sum())


def pick(host):
    g = dict(np.load(os.path.join(HERE, "rules.npz")))
    want = {"check": 3, "mated": 1, "black": 2, "flying": 2, "plain": 4}
    out = []
    for i in range(7, len(g["boards"]), 7):   # 0 is the start position
        b, s = g["boards"][i], int(g["side"][i])
        if (b == 1).sum() != 1 or (b == 8).sum() != 1 or M.attacked(b, 1 - s):
            continue   # a position of a king-capture game that Xiangqi rules never reach
        moves, flags = M.kingsafe(b, s)
        kb = kings_between(b)
        tag = ("mated" if flags & M.NO_SAFE_MOVE else "check" if flags & M.IN_CHECK else "flying" if kb is not None and kb <= 1 else
               "black" if s else "plain")
        if want[tag]:
            want[tag] -= 1
            out.append(("rules.npz[%d]" % i, b, s, 3, tag))
        if not any(want.values()):
            break
    assert not any(want.values()), want
    ob, os_ = open_boards(60, 5)
    n = 0
    for i in range(len(ob)):
        if n < 3 and not M.attacked(ob[i], 1 - int(os_[i])) and len(M.kingsafe(ob[i], int(os_[i]))[0]) >= 80:
            out.append(("open_boards(60, 5)[%d]" % i, ob[i], int(os_[i]), 2, "open"))
            n += 1
    assert n == 3
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        host = perft_host.load(tmp)
        b0 = O.fen_to_board(O.START_FEN)
        start = split_perft(host, b0, 0, 5)
        for k, v in START.items():
            assert [int(x) for x in start[k]] == v, (k, start[k], v)
        d6 = START_DEPTH6
        if "--depth6" in sys.argv:
            d6 = int(split_perft(host, b0, 0, 6, stats=False)["nodes"][6])
            assert d6 == START_DEPTH6, d6
        doc = {"columns": list(perft_host.COLUMNS),
               "start": dict(board=[int(x) for x in b0], side=0, depth=5, nodes_depth6=d6, **{k: [int(x) for x in v] for k, v in start.items()}),
               "positions": []}
        for source, b, s, depth, tag in pick(host):
            t = host(b, s, depth)
            doc["positions"].append(dict(source=source, tag=tag, board=[int(x) for x in b], side=s, depth=depth,
                                         **{k: [int(x) for x in v] for k, v in t.items()}))
    P = doc["positions"]
    assert len(P) >= 12
    assert sum(p["checks"][0] for p in P) >= 3                                    # roots in check
    assert any(p["mates"][0] and p["nodes"][1:] == [0] * p["depth"] for p in P)   # a root without a safe move: perft 1, 0, 0 ...
    assert any(p["side"] == 1 for p in P)                                         # black to move
    assert any(p["tag"] == "flying" for p in P)                                   # a king the other king can fly at
    for k in ("captures", "checks", "mates"):
        assert sum(sum(p[k][1:]) for p in P) > 0, k                               # every column is exercised below the roots
    with open(os.path.join(HERE, "perft.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print("perft.json: the start position to depth 5 and %d positions" % len(P))
    for p in P:
        print("  %-24s %-6s side %d depth %d nodes %s checks %s mates %s" % (p["source"], p["tag"], p["side"], p["depth"], p["nodes"], p["checks"], p["mates"]))


if __name__ == "__main__":
    main()
