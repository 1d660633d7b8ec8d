"""Forced mates under Xiangqi rules: is there one within N plies, and what is the line?

    python -m cchess_zero_amd.mate --fen "<fen>" [--fen "<fen>" ...] [--fen-file F] [--plies 9] [--all-moves] [--node-limit N]
                                   [--notation iccs|wxf|chinese]

prints one JSON object per position: fen, status ("mate", "none", "bad_root", "node_limit"), mate_in (the attacker's moves,
(dist + 1) // 2; null without a mate), plies (dist; null without a mate), pv (the line, every move written in the position it
is played in), nodes (positions made for this root) and seconds (of the whole call, the same for every position).

The solver is Rules.mate: the side to move attacks, by default with checking moves only (the continuous-check mate of Xiangqi
puzzles; --all-moves lets it play every king-safe move), the defender has every king-safe move, and all positions are solved
in one depth-first pass on the GPU.  Repetition and perpetual-check rules are not applied inside the proof."""
import argparse
import json
import time

import numpy as np

from .notation import fen_to_position, line_text

STATUS = ("none", "mate", "bad_root", "node_limit")   # Rules.mate's status 0 .. 3


def solve(rules, positions, plies, all_moves=False, node_limit=None, notation="iccs"):
    """positions: FEN strings or (board uint8[90], side[, restrict round]) tuples -> per position dict(status, mate_in, plies,
    pv, nodes, seconds), by one Rules.mate call on `rules`."""
    pos = [fen_to_position(p) if isinstance(p, str) else p for p in positions]
    if not pos:
        return []
    boards = np.stack([np.asarray(p[0], np.uint8).reshape(90) for p in pos])
    side = np.array([1 if p[1] else 0 for p in pos], np.uint8)
    start = time.perf_counter()
    res = rules.mate(boards, side, plies, attacker="all" if all_moves else "checks", node_limit=node_limit)
    seconds = time.perf_counter() - start
    out = []
    for i in range(len(pos)):
        found = int(res["status"][i]) == 1
        d = int(res["dist"][i])
        line = [int(l) for l in res["pv"][i] if int(l) != 0xFFFF]
        out.append(dict(status=STATUS[int(res["status"][i])], mate_in=(d + 1) // 2 if found else None, plies=d if found else None,
                        pv=line_text(boards[i], side[i], line, notation) if found else [], nodes=int(res["nodes"][i]), seconds=round(seconds, 6)))
    return out


def main(argv=None, rules=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.mate",
                                 description="Forced mates of Xiangqi positions (continuous-check by default); one JSON object per position.")
    ap.add_argument("--fen", action="append", default=[], help="a position as standard Xiangqi FEN (may be given more than once)")
    ap.add_argument("--fen-file", default=None, help="a file with one FEN per line")
    ap.add_argument("--plies", type=int, default=9, help="the horizon: odd, 1 .. 15 (default 9: mate in five)")
    ap.add_argument("--all-moves", action="store_true", help="the attacker may play every king-safe move, not only checks")
    ap.add_argument("--node-limit", type=int, default=None, help="stop expanding once this many positions have been made")
    ap.add_argument("--notation", choices=("iccs", "wxf", "chinese"), default="iccs", help="how the moves of the output are written (default: ICCS)")
    args = ap.parse_args(argv)
    fens = list(args.fen)
    if args.fen_file:
        fens += [l.strip() for l in open(args.fen_file) if l.strip()]
    if not fens:
        ap.error("no position: give --fen or --fen-file")
    if args.plies < 1 or args.plies > 15 or args.plies % 2 == 0:
        ap.error("--plies is odd, 1 .. 15")
    if args.node_limit is not None and args.node_limit < 1:
        ap.error("--node-limit is at least 1")
    try:
        pos = [fen_to_position(f) for f in fens]
    except ValueError as e:
        ap.error(str(e))
    if rules is None:
        from .rules import Rules
        rules = Rules()
    rows = [dict(fen=f, **r) for f, r in zip(fens, solve(rules, pos, args.plies, args.all_moves, args.node_limit, args.notation))]
    for r in rows:
        print(json.dumps(r, ensure_ascii=args.notation != "chinese"), flush=True)
    return rows


if __name__ == "__main__":
    main()
