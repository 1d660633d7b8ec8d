"""Perft under Xiangqi rules on the GPU (Rules.perft: movegen_kingsafe -> successors, ply by ply); prints one JSON line.

    python -m cchess_zero_amd.perft --depth 5 --stats
    python -m cchess_zero_amd.perft --depth 4 --divide --state RNBAKABNR/9/1C5C1/P1P1P1P1P/9/9/p1p1p1p1p/1c5c1/9/rnbakabnr --player w

The start position's published table is 44, 1 920, 79 666, 3 290 240, 133 312 995, 5 392 831 844."""
import argparse
import json
import time

import torch

from .notation import START_STATE, player_to_side, state_to_board
from .rules import Rules


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.perft", description="Perft under Xiangqi rules on the GPU; prints one JSON line.")
    ap.add_argument("--depth", type=int, required=True, help="plies")
    ap.add_argument("--state", default=START_STATE, help="the position, as the reference writes a state (default: the start position)")
    ap.add_argument("--player", choices=("w", "b"), default="w", help="the side to move")
    ap.add_argument("--stats", action="store_true", help="captures, checks and mates beside the nodes (the last ply is made, not counted)")
    ap.add_argument("--divide", action="store_true", help="the nodes of --depth split by the first move")
    ap.add_argument("--chunk", type=int, default=None, help="parents per slice of the depth-first walk (default Rules.PERFT_CHUNK)")
    args = ap.parse_args(argv)
    if args.depth < (1 if args.divide else 0):
        ap.error("--depth >= %d" % (1 if args.divide else 0))
    rules = Rules()
    board, side = state_to_board(args.state), player_to_side(args.player)
    rules.perft(board, [side], min(args.depth, 1))   # the library and the kernels are loaded before the clock starts
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = rules.perft(board, [side], args.depth, stats=args.stats, chunk=args.chunk)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    d = dict(state=args.state, player=args.player, depth=args.depth, chunk=args.chunk or Rules.PERFT_CHUNK)
    d.update({k: [int(x) for x in v[0]] for k, v in out.items()})
    d.update(seconds=round(seconds, 4), nodes_per_s=round(float(out["nodes"][0].sum()) / max(seconds, 1e-9), 1))
    if args.divide:
        d["divide"] = rules.divide(board, side, args.depth)
    print(json.dumps(d), flush=True)
    return d


if __name__ == "__main__":
    main()
