#!/usr/bin/env python3
"""Throughput of the stand-alone rules kernels (K1 move generation, K2 make-move, K3 planes) on a batch large
enough to fill the chip: positions/s and the HBM traffic that implies (SURVEY §8d quotes K1 at 312 B/position for
a nibble board + mask; this ABI moves 90 B board + 1 B side in, 256 B ordered list + 264 B mask + 2 B count out).
usage: python tools/rules_bench.py [N positions, default 1048576]
       python tools/rules_bench.py --kingsafe [N]     the king-safe generator (cz_movegen_kingsafe) on N positions of
           rules.random_positions against (a) the pseudo-legal kernels on the same positions and (b) the same answer composed from
           cz_movegen + cz_apply_move + cz_movegen + torch; one JSON line at the end
       python tools/rules_bench.py --threats [N]      the threat kernel of the chase rule (cz_threats) beside the king-safe
           generator's flags-only and list forms on the same N positions, in the same run; one JSON line at the end
       python tools/rules_bench.py --successors [N]   cz_successors on the first N positions of the start position's depth-4
           frontier (3 290 240 positions) with their king-safe lists: time and achieved store bandwidth; one JSON line at the end
       python tools/rules_bench.py --replay [G]       cz_games_replay on G (default 8192) games of games.random_games under each rule
           level against the same answer from the ply-by-ply path that made them (one move-list launch and one cz_apply_move launch
           per ply, games.ply_by_ply_replay), both timed in the same run, alternating; one JSON line at the end.  Then the
           notation leg (--replay-notation [G]: that leg alone): the same games as labels through cz_games_replay and as WXF
           tokens through cz_games_read, alternating, and a host decode in Python on a 256-game sample, scaled; one JSON line
       python tools/rules_bench.py --checks [N]       the checking-move generator (cz_movegen_checks) on N positions of
           rules.random_positions against the composition it replaces (cz_movegen_kingsafe list -> cz_successors -> the flags-only
           form on every child -> boolean compaction in torch), both in the same run; one JSON line at the end
       python tools/rules_bench.py --mate [N]         Rules.mate ("checks" mode) at plies 5 and 9 on N (default 65 536) positions
           of rules.random_positions: roots/s and nodes/s; one JSON line at the end
       python tools/rules_bench.py --tablebase SIG    the retrograde build of one endgame table (Tablebase.build): wall time, passes
           and entries per second of every pass; then an early pass (the first: every undecided lane is live) and a late one (the
           last that decides anything: most groups are skipped) as the fused cz_tb_pass against the same pass composed from
           cz_tb_boards -> cz_movegen_kingsafe -> cz_successors -> Tablebase.probe -> a torch segment reduction, from the same
           snapshot of the table, alternating in one run; one JSON line at the end
       python tools/rules_bench.py --tablebase-set SIG    the mixed probe: the closure of SIG is built, 65 536 legal positions are
           drawn evenly from all of its tables and shuffled, and Tablebase.probe (host grouping, one cz_tb_probe per signature) is
           timed against Tablebase.probe_set (one k_tb_probe_set launch) on them — device events, one warm-up, the two forms
           alternating three times, the answers compared; then the one launch on 8192 start positions, all misses: what self-play
           pays per ply with a table set attached; one JSON line at the end
       python tools/rules_bench.py --book             the opening book's kernels (csrc/cz_book.hip): cz_book_keys on 1 M positions
           against the composed path (the boards flipped in torch, two cz_hash launches, torch.minimum on the flipped-sign keys),
           cz_book_probe on 65 536 positions against a book of about 1 M entries against the composed keys followed by
           torch.searchsorted — device events, one warm-up call, the two forms alternating, the answers compared — and Book.build
           on the records of 65 536 random games, end to end (host clock); one JSON line at the end
       python tools/rules_bench.py --repetition-moves [N]   cz_repetition_moves (fold 3, chase records given) on N (default 4096)
           mid-game positions of random king-safe games with the 40 plies before them as their records, against the same answer
           composed from the public calls (king-safe lists -> cz_successors -> king-safe lists of the children -> cz_successors
           -> cz_hash / flags / cz_threats of every child and grandchild -> extended records -> cz_repetition_chase -> a torch
           reduction) on the first min(N, 1024) of them — the host clock around a synchronise for both forms (and device events
           around the fused call), one warm-up each, the two forms alternating, the answers compared; one JSON line.  Then the same
           on games whose last 16 plies shuffle (each side takes its last move back when it may): positions that repeat, the hit
           path; one JSON line.  Then the avoid step: a match on 8192 slots (random openings, a constant net, 8 playouts), 24 plies
           with cz_match_set_avoid on and 24 with it off, device events around every cz_match_choose; one JSON line at the end"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (synthetic position generator)
from cchess_zero_amd.engine import Context  # noqa: E402
from cchess_zero_amd.rules import Rules  # noqa: E402

KINGSAFE = "--kingsafe" in sys.argv
THREATS = "--threats" in sys.argv
SUCCESSORS = "--successors" in sys.argv
REPLAY = "--replay" in sys.argv
REPLAY_NOTATION = "--replay-notation" in sys.argv
CHECKS = "--checks" in sys.argv
BOOK = "--book" in sys.argv
MATE = "--mate" in sys.argv
REPMOVES = "--repetition-moves" in sys.argv
TABLEBASE = None
if "--tablebase" in sys.argv:
    _at = sys.argv.index("--tablebase")
    if _at + 1 >= len(sys.argv):
        sys.exit("--tablebase needs a signature such as KR-KAABB")
    TABLEBASE = sys.argv[_at + 1]
    del sys.argv[_at:_at + 2]
TABLEBASE_SET = None
if "--tablebase-set" in sys.argv:
    _at = sys.argv.index("--tablebase-set")
    if _at + 1 >= len(sys.argv):
        sys.exit("--tablebase-set needs a signature such as KR-KAA")
    TABLEBASE_SET = sys.argv[_at + 1]
    del sys.argv[_at:_at + 2]
_args = [a for a in sys.argv[1:] if a not in ("--kingsafe", "--threats", "--successors", "--replay", "--replay-notation", "--checks", "--mate", "--book", "--repetition-moves")]
N = int(_args[0]) if _args else (8192 if REPLAY or REPLAY_NOTATION else 1 << 16 if MATE else 4096 if REPMOVES else 1 << 20)
ctx = Context(1, 2, 0)
rules = Rules(ctx)


def kingsafe_leg():
    """Median of 25 launches (device events, 3 warm-up launches) per form; (b) is a chain of launches: host clock around a
    synchronise, median of 5, on the first 131 072 positions (it holds ~35 child boards and masks per position)."""
    import json
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.rules import random_positions
    boards, side, _ = random_positions(rules, N, seed=17)

    def median_ms(fn, launches=25, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        return ts[len(ts) // 2], ts[0], ts[-1]

    forms = {
        "kingsafe_flags_only": lambda: rules.in_check(boards, side),
        "kingsafe_set_only": lambda: rules.movegen_kingsafe(boards, side, want_moves=False),
        "kingsafe_list_and_set": lambda: rules.movegen_kingsafe(boards, side, pad=False),
        "pseudo_mask_kernel": lambda: rules.movegen(boards, side, want_moves=False),
        "pseudo_list_and_mask_kernel": lambda: rules.movegen(boards, side, pad=False),
    }
    out = {"positions": N}
    for name, fn in forms.items():
        med, lo, hi = median_ms(fn)
        out[name] = dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), positions_per_s=round(N / med * 1e3))
        print("%-28s: median %.3f ms (min %.3f, max %.3f) = %.3f G positions/s" % (name, med, lo, hi, N / med / 1e6))
    # (b) today's kernels composed: every pseudo-legal move applied to a copy of its position, the replies' set, and the bit
    # test "does a reply land on the mover's king" in torch
    M = min(N, 131072)
    sd = tables()["srcdst"].astype(np.int64)
    onto = np.zeros((90, 66), np.int64)
    for l in range(len(sd)):
        onto[sd[l] >> 8, l >> 5] |= 1 << (l & 31)
    onto = torch.from_numpy(onto.astype(np.uint32).view(np.int32)).cuda()

    def composed():
        b, s = boards[:M], side[:M]
        mv, cnt, _ = rules.movegen(b, s, want_mask=False)
        c = cnt.to(torch.int64) & 0xFFFF
        parent = torch.repeat_interleave(torch.arange(M, device=b.device), c)
        first = torch.cumsum(c, 0) - c
        k = torch.arange(parent.numel(), device=b.device) - first[parent]
        lab = mv[parent, k].contiguous()
        cb, cs = b[parent].contiguous(), s[parent].contiguous()
        rules.apply_move(cb, cs, lab)
        _, _, reply = rules.movegen(cb, cs, want_moves=False)
        king = (cb == torch.where(s[parent] == 0, 1, 8).to(torch.uint8).unsqueeze(1))
        has_king, ksq = king.any(1), king.to(torch.uint8).argmax(1)
        unsafe = has_king & ((reply & onto[ksq]) != 0).any(1)
        safe_count = torch.zeros(M, dtype=torch.int64, device=b.device).index_add_(0, parent, (~unsafe).to(torch.int64))
        return safe_count, parent.numel()

    sc, children = composed()
    _, kc, _, _ = rules.movegen_kingsafe(boards[:M], side[:M], want_moves=False)
    assert torch.equal(sc, kc.to(torch.int64) & 0xFFFF), "the composed answer and cz_movegen_kingsafe disagree"
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        composed()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    out["composed"] = dict(positions=M, child_positions=children, ms=round(ts[2], 3), positions_per_s=round(M / ts[2] * 1e3))
    print("%-28s: median %.3f ms for %d positions (%d child positions) = %.4f G positions/s" % ("composed (b)", ts[2], M, children, M / ts[2] / 1e6))
    ks = out["kingsafe_set_only"]["positions_per_s"]
    out["set_vs_pseudo_mask_kernel"] = round(ks / out["pseudo_mask_kernel"]["positions_per_s"], 4)
    out["list_and_set_vs_pseudo_list_kernel"] = round(out["kingsafe_list_and_set"]["positions_per_s"] / out["pseudo_list_and_mask_kernel"]["positions_per_s"], 4)
    out["set_vs_composed"] = round(ks / out["composed"]["positions_per_s"], 2)
    print(json.dumps(out), flush=True)


def threats_leg():
    """Median of 25 launches (device events, 3 warm-up launches) per kernel, all on the same positions of random_positions."""
    import json
    from cchess_zero_amd.rules import random_positions
    boards, side, _ = random_positions(rules, N, seed=17)
    forms = {
        "kingsafe_flags_only": lambda: rules.in_check(boards, side),
        "threats": lambda: rules.threats(boards, side),
        "kingsafe_list": lambda: rules.movegen_kingsafe(boards, side, want_mask=False, pad=False),
        "kingsafe_list_and_set": lambda: rules.movegen_kingsafe(boards, side, pad=False),
    }
    out = {"positions": N}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[name] = dict(ms=round(ts[12], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), positions_per_s=round(N / ts[12] * 1e3))
        print("%-24s: median %.3f ms (min %.3f, max %.3f) = %.3f G positions/s" % (name, ts[12], ts[0], ts[-1], N / ts[12] / 1e6))
    rec = rules.threats(boards, side)
    out["positions_with_a_threat"] = int(((rec[:, 0] | rec[:, 1]) != 0).sum().item())
    print(json.dumps(out), flush=True)


def checks_leg():
    """cz_movegen_checks (list, CZ_MOVES_NO_PAD; and the count / flags form) on all N positions: median of 25 launches (device
    events, 3 warm-up launches).  The composition it replaces is a chain of launches that holds ~40 child boards per position,
    so it runs on the first 131 072 positions, host clock around a synchronise, median of 5 — and so does cz_movegen_checks
    once more, timed the same way on the same positions, which is the pair the ratio is taken from.  Before anything is
    timed the two answers (list and count) are asserted equal."""
    import json
    from cchess_zero_amd._lib import POS_IN_CHECK
    from cchess_zero_amd.rules import random_positions
    boards, side, _ = random_positions(rules, N, seed=17)
    M = min(N, 131072)
    b, s = boards[:M].contiguous(), side[:M].contiguous()

    def composed():
        mv, cnt, _, _ = rules.movegen_kingsafe(b, s, want_mask=False, pad=False)
        cb, cs, _, par, label = rules.successors(b, s, mv, cnt)
        keep = rules.in_check(cb, cs) & POS_IN_CHECK != 0
        par, label = par[keep].to(torch.int64), label[keep]
        count = torch.zeros(M, dtype=torch.int64, device=b.device).index_add_(0, par, torch.ones_like(par))
        first = torch.cumsum(count, 0) - count
        rows = torch.full((M, 128), -1, dtype=torch.int16, device=b.device)
        rows[par, torch.arange(par.numel(), device=b.device) - first[par]] = label
        return rows, count, cb.shape[0]

    rows, count, children = composed()
    mv, cnt, _ = rules.checks(b, s)
    assert torch.equal(cnt.to(torch.int64), count) and torch.equal(mv, rows), "the composed answer and cz_movegen_checks disagree"
    out = {"positions": N, "checks_per_position": round(float(count.sum().item()) / M, 3), "positions_with_a_check": round(float((count > 0).sum().item()) / M, 4)}
    forms = {"checks_list": lambda: rules.checks(boards, side, pad=False), "checks_count_only": lambda: rules.checks(boards, side, want_moves=False),
             "kingsafe_list": lambda: rules.movegen_kingsafe(boards, side, want_mask=False, pad=False)}
    for name, fn in forms.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[name] = dict(ms=round(ts[12], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), positions_per_s=round(N / ts[12] * 1e3))
        print("%-18s: median %.3f ms (min %.3f, max %.3f) = %.3f G positions/s" % (name, ts[12], ts[0], ts[-1], N / ts[12] / 1e6))
    for name, fn in (("composed", composed), ("checks_list_same_positions", lambda: rules.checks(b, s, pad=False))):
        fn()
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts.sort()
        out[name] = dict(positions=M, ms=round(ts[2], 3), min_ms=round(ts[0], 3), max_ms=round(ts[-1], 3), positions_per_s=round(M / ts[2] * 1e3))
        print("%-28s: median %.3f ms (min %.3f, max %.3f) for %d positions = %.4f G positions/s" % (name, ts[2], ts[0], ts[-1], M, M / ts[2] / 1e6))
    out["composed"]["child_positions"] = children
    out["checks_vs_composed"] = round(out["composed"]["ms"] / out["checks_list_same_positions"]["ms"], 2)
    print(json.dumps(out), flush=True)


def mate_leg():
    """Rules.mate in "checks" mode on N positions of random_positions at plies 5 and 9: host clock around the call (it ends by
    copying its answers to the host), one warm-up call at plies 1, then the median of 3 calls per horizon."""
    import json
    from cchess_zero_amd.rules import random_positions
    boards, side, _ = random_positions(rules, N, seed=17)
    rules.mate(boards, side, 1)
    out = {"positions": N}
    for plies in (5, 9):
        ts = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = rules.mate(boards, side, plies)
            ts.append(time.perf_counter() - t0)
        ts.sort()
        nodes = int(res["nodes"].sum())
        out["plies_%d" % plies] = dict(s=round(ts[1], 4), min_s=round(ts[0], 4), max_s=round(ts[-1], 4), mates=int((res["status"] == 1).sum()),
                                       bad_roots=int((res["status"] == 2).sum()), nodes=nodes, roots_per_s=round(N / ts[1]), nodes_per_s=round(nodes / ts[1]))
        print("mate plies %d: median %.3f s (min %.3f, max %.3f) for %d roots, %d mates, %d nodes = %.1f k roots/s, %.2f M nodes/s"
              % (plies, ts[1], ts[0], ts[-1], N, out["plies_%d" % plies]["mates"], nodes, N / ts[1] / 1e3, nodes / ts[1] / 1e6))
    print(json.dumps(out), flush=True)


def successors_leg():
    """Median of 25 launches (device events, 3 warm-up launches) of the bare C call into buffers allocated once: all five outputs,
    and the boards alone.  The lists, the offsets and their sum are made before the clock starts."""
    import json
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import _ptr
    from cchess_zero_amd.rules import START_BOARD
    boards, side = torch.from_numpy(START_BOARD[None].copy()).cuda(), torch.zeros(1, dtype=torch.uint8, device="cuda")
    for _ in range(4):
        mv, cnt, _, _ = rules.movegen_kingsafe(boards, side, want_mask=False, pad=False)
        boards, side = rules.successors(boards, side, mv, cnt)[:2]
    boards, side = boards[:N].contiguous(), side[:N].contiguous()
    n = boards.shape[0]
    mv, cnt, _, _ = rules.movegen_kingsafe(boards, side, want_mask=False, pad=False)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(cnt.to(torch.int64), 0)
    T = int(offsets[-1].item())
    offsets = offsets.to(torch.int32)
    ob = torch.empty((T, 90), dtype=torch.uint8, device="cuda")
    o1, o2 = torch.empty(T, dtype=torch.uint8, device="cuda"), torch.empty(T, dtype=torch.uint8, device="cuda")
    o4, o5 = torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty(T, dtype=torch.int16, device="cuda")
    ctx.bind_stream()
    out = {"parents": n, "children": T}
    for name, rest, width in (("all_outputs", (o1, o2, o4, o5), 98), ("boards_only", (None,) * 4, 90)):
        fn = lambda: check(lib().cz_successors(ctx.h, _ptr(boards), _ptr(side), n, _ptr(mv), _ptr(offsets), T, _ptr(ob), *[_ptr(x) for x in rest]))
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        out[name] = dict(ms=round(ts[12], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), children_per_s=round(T / ts[12] * 1e3),
                         store_TB_per_s=round(T * width / ts[12] / 1e9, 3))
        print("%-12s: median %.3f ms (min %.3f, max %.3f) for %d parents, %d children = %.2f G children/s, %.2f TB/s of stores"
              % (name, ts[12], ts[0], ts[-1], n, T, T / ts[12] / 1e6, T * width / ts[12] / 1e9))
    print(json.dumps(out), flush=True)


def replay_leg(max_ply=160):
    """Per rule level: N games of random_games (U[0, max_ply] plies, less where a game ends before).  The fused replay is the bare
    C call into buffers allocated once, the games sorted by length as GameReplayer sorts them (and once more in the order they
    came: what the sort is worth); the yardstick is ply_by_ply_replay on the same device arrays.  Device events, 3 warm-up
    launches, then 25 rounds of fused / unsorted / ply by ply one after the other; medians.  The final boards of all three are
    asserted equal to the ones random_games reached before anything is timed."""
    import json
    from cchess_zero_amd import games as G
    from cchess_zero_amd._lib import check, lib
    from cchess_zero_amd.engine import _ptr
    out = {"games": N, "max_ply": max_ply}
    for level, r in (("capture", 0), ("xiangqi", 1)):
        rg = G.random_games(level, N, 23, max_ply, engine_rules=rules)
        lens, plies = rg["lens"].astype(np.int64), int(rg["lens"].sum())
        offset = np.concatenate([[0], np.cumsum(lens)[:-1]])
        rec = torch.empty((plies, 608), dtype=torch.uint8, device="cuda")
        valid, status = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
        flags, fside = torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
        fboards = torch.empty((N, 90), dtype=torch.uint8, device="cuda")
        zero = torch.zeros(N, dtype=torch.int8, device="cuda")
        forms = {}
        for name, order in (("fused_sorted", np.argsort(lens, kind="stable")), ("fused_input_order", np.arange(N))):
            mv = ctx.tensor(rg["moves"][order], torch.int16)
            ln, off = ctx.tensor(lens[order], torch.int32), ctx.tensor(offset[order], torch.int32)
            forms[name] = (lambda mv=mv, ln=ln, off=off: check(lib().cz_games_replay(ctx.h, None, None, _ptr(mv), max_ply, _ptr(ln), _ptr(zero), N, r, _ptr(off),
                                                                                     plies, _ptr(rec), _ptr(valid), _ptr(status), _ptr(flags), _ptr(fboards),
                                                                                     _ptr(fside))), order)
        d_mv, d_ln = ctx.tensor(rg["moves"], torch.int16), ctx.tensor(rg["lens"], torch.int32)
        ctx.bind_stream()
        for name, (fn, order) in forms.items():
            fn()
            torch.cuda.synchronize()
            assert (status == 0).all() and np.array_equal(fboards.cpu().numpy(), rg["final_boards"][order]) and np.array_equal(valid.cpu().numpy(), lens[order]), name
        v, fb, _ = G.ply_by_ply_replay(level, d_mv, d_ln, engine_rules=rules)
        assert np.array_equal(fb.cpu().numpy(), rg["final_boards"]) and np.array_equal(v.cpu().numpy(), lens), "ply by ply"
        timed_forms = {k: f for k, (f, _) in forms.items()}
        timed_forms["ply_by_ply"] = lambda: G.ply_by_ply_replay(level, d_mv, d_ln, engine_rules=rules)
        ts = {k: [] for k in timed_forms}
        for it in range(3 + 25):
            for name, fn in timed_forms.items():
                ctx.bind_stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    ts[name].append(e0.elapsed_time(e1))
        o = {"plies": plies, "mean_len": round(plies / N, 2), "max_len": int(lens.max())}
        for name, t in ts.items():
            t.sort()
            o[name] = dict(ms=round(t[12], 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4), plies_per_s=round(plies / t[12] * 1e3))
            print("%-8s %-18s: median %.3f ms (min %.3f, max %.3f) for %d games, %d plies = %.2f M plies/s"
                  % (level, name, t[12], t[0], t[-1], N, plies, plies / t[12] / 1e3))
        o["fused_vs_ply_by_ply"] = round(o["ply_by_ply"]["ms"] / o["fused_sorted"]["ms"], 2)
        o["sorted_vs_input_order"] = round(o["fused_input_order"]["ms"] / o["fused_sorted"]["ms"], 3)
        out[level] = o
    print(json.dumps(out), flush=True)


def wxf_tokens(boards, side, labels, srcdst):
    """The writer's rule (cchess_zero_amd/notation.py: move_token) for n plies at once: boards uint8 [n, 90] before the move, side
    [n], labels [n] -> uint32 [n].  Standard material only (no side has three of a kind that is not the pawn)."""
    n = len(labels)
    ar, side = np.arange(n), side.astype(np.int64)
    sq = srcdst[labels].astype(np.int64)
    frm, to = sq & 0xFF, sq >> 8
    fy, fx, ty, tx = frm // 9, frm % 9, to // 9, to % 9
    grid = boards.reshape(n, 10, 9)
    pc = boards[ar, frm]
    kind = pc.astype(np.int64) - 7 * side                       # K A R E H P C = 1 .. 7
    same = grid[ar, :, fx] == pc[:, None]                      # [n, 10]: the kind on the source's file
    cnt = same.sum(axis=1)
    ys = np.arange(10)[None, :]
    ahead = (same & np.where(side[:, None] == 1, ys < fy[:, None], ys > fy[:, None])).sum(axis=1)
    fileno = lambda x: np.where(side == 1, x + 1, 9 - x)
    dy = np.where(side == 1, fy - ty, ty - fy)
    digit = (cnt == 1) | (kind == 2) | (kind == 4)
    b1 = np.where(digit, ord("0") + fileno(fx), np.where(ahead == 0, ord("+"), np.where(ahead == cnt - 1, ord("-"), ord("a") + ahead)))
    doubled = ((grid == pc[:, None, None]).sum(axis=1) >= 2).sum(axis=1) > 1
    b0 = np.where((kind == 6) & ~digit & doubled, ord("0") + fileno(fx), np.array([0] + [ord(c) for c in "KAREHPC"])[kind])
    leaper = (kind == 2) | (kind == 4) | (kind == 5)
    b2 = np.where(dy == 0, ord("="), np.where(dy > 0, ord("+"), ord("-")))
    b3 = ord("0") + np.where((dy == 0) | leaper, fileno(tx), np.abs(dy))
    return (b0 | b1 << 8 | b2 << 16 | b3 << 24).astype(np.uint32)


def notation_leg(max_ply=160, sample=256):
    """Per rule level: the N games of replay_leg, sorted by length, as labels through cz_games_replay (the path before
    cz_games_read) and as WXF tokens through cz_games_read with labels_out: device events, 3 warm-up launches, then 25 rounds of
    one after the other; medians.  The tokens are written from the label replay's records (wxf_tokens, checked against
    notation.move_token on a sample); before anything is timed the token replay's final boards and decoded labels are asserted
    equal to the games'.  The host leg steps `sample` of the games through the C oracle's lists in Python and names every token
    with tests/notation_model.py's matcher, timed on the host clock and scaled to N games by plies."""
    import json
    from cchess_zero_amd import games as G
    from cchess_zero_amd import notation
    from cchess_zero_amd._lib import check, lib, tables
    from cchess_zero_amd.engine import _ptr
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import games_model as GM
    import notation_model as NM
    from oracle import oracle as O
    srcdst = tables()["srcdst"]
    out = {"games": N, "max_ply": max_ply}
    for level, r in (("capture", 0), ("xiangqi", 1)):
        rg = G.random_games(level, N, 23, max_ply, engine_rules=rules)
        order = np.argsort(rg["lens"], kind="stable")
        moves, lens = rg["moves"][order], rg["lens"][order].astype(np.int64)
        plies = int(lens.sum())
        offset = np.concatenate([[0], np.cumsum(lens)[:-1]])
        rec = torch.empty((plies, 608), dtype=torch.uint8, device="cuda")
        valid, status = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
        flags, fside = torch.empty(N, dtype=torch.uint8, device="cuda"), torch.empty(N, dtype=torch.uint8, device="cuda")
        fboards = torch.empty((N, 90), dtype=torch.uint8, device="cuda")
        labels_out = torch.empty((N, max_ply), dtype=torch.int16, device="cuda")
        zero = torch.zeros(N, dtype=torch.int8, device="cuda")
        mv, ln, off = ctx.tensor(moves, torch.int16), ctx.tensor(lens, torch.int32), ctx.tensor(offset, torch.int32)
        as_labels = lambda: check(lib().cz_games_replay(ctx.h, None, None, _ptr(mv), max_ply, _ptr(ln), _ptr(zero), N, r, _ptr(off), plies, _ptr(rec),
                                                        _ptr(valid), _ptr(status), _ptr(flags), _ptr(fboards), _ptr(fside)))
        ctx.bind_stream()
        as_labels()
        torch.cuda.synchronize()
        assert (status == 0).all() and np.array_equal(fboards.cpu().numpy(), rg["final_boards"][order]), "labels"
        played = moves[np.arange(max_ply)[None, :] < lens[:, None]].astype(np.int64)      # row-major: the records' order
        tok = np.empty(plies, np.uint32)
        for lo in range(0, plies, 1 << 20):
            head = rec[lo:lo + (1 << 20), :91].cpu().numpy()
            tok[lo:lo + (1 << 20)] = wxf_tokens(np.ascontiguousarray(head[:, :90]), head[:, 90], played[lo:lo + (1 << 20)], srcdst)
        for i in np.random.default_rng(1).integers(0, plies, 2000):
            h = rec[int(i), :91].cpu().numpy()
            assert int(tok[i]) == notation.move_token(h[:90], int(h[90]), int(played[i])), (i, notation.token_text(tok[i]))
        tokens = np.full((N, max_ply), 0xFFFF, np.uint32)
        tokens[np.arange(max_ply)[None, :] < lens[:, None]] = tok
        d_tok = ctx.tensor(tokens, torch.int32)
        as_tokens = lambda: check(lib().cz_games_read(ctx.h, None, None, _ptr(d_tok), max_ply, _ptr(ln), _ptr(zero), N, r, _ptr(off), plies, _ptr(rec),
                                                      _ptr(valid), _ptr(status), _ptr(flags), _ptr(fboards), _ptr(fside), _ptr(labels_out)))
        want_rec = rec[:min(plies, 1 << 16)].clone()
        rec.fill_(0xA5)
        as_tokens()
        torch.cuda.synchronize()
        assert (status == 0).all() and np.array_equal(fboards.cpu().numpy(), rg["final_boards"][order]) and np.array_equal(valid.cpu().numpy(), lens), "tokens"
        assert np.array_equal(labels_out.cpu().numpy().view(np.uint16), moves) and torch.equal(rec[:len(want_rec)], want_rec), "tokens decode to the labels"
        timed_forms = {"labels_cz_games_replay": as_labels, "wxf_cz_games_read": as_tokens}
        ts = {k: [] for k in timed_forms}
        for it in range(3 + 25):
            for name, fn in timed_forms.items():
                ctx.bind_stream()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if it >= 3:
                    ts[name].append(e0.elapsed_time(e1))
        o = {"plies": plies, "text_tokens": int((tok >= 65536).sum()), "ordinal_tokens": int(np.isin((tok >> 8) & 0xFF, [ord(c) for c in "+-abcde"]).sum())}
        for name, t in ts.items():
            t.sort()
            o[name] = dict(ms=round(t[12], 4), min_ms=round(t[0], 4), max_ms=round(t[-1], 4), plies_per_s=round(plies / t[12] * 1e3))
            print("%-8s %-24s: median %.3f ms (min %.3f, max %.3f) for %d games, %d plies = %.2f M plies/s"
                  % (level, name, t[12], t[0], t[-1], N, plies, plies / t[12] / 1e3))
        # the host decode: a Python board stepped through every ply of `sample` games spread over the lengths
        pick = np.linspace(0, N - 1, min(sample, N)).astype(np.int64)
        t0, done = time.perf_counter(), 0
        for g in pick:
            b, s = GM.start_board(), 0
            for i in range(int(lens[g])):
                named = NM.Position(b, s, GM.legal_list(b, s, r)).matching(int(tokens[g, i]))
                assert named == [int(moves[g, i])]
                b, s = O.apply_move(b, named[0])[0], s ^ 1
                done += 1
        host_s = time.perf_counter() - t0
        o["host_python_decode"] = dict(sample_games=len(pick), sample_plies=done, sample_s=round(host_s, 3), us_per_ply=round(host_s / max(done, 1) * 1e6, 1),
                                       scaled_s=round(host_s / max(done, 1) * plies, 2))
        o["read_vs_replay"] = round(o["wxf_cz_games_read"]["ms"] / o["labels_cz_games_replay"]["ms"], 3)
        o["host_decode_vs_read"] = round(o["host_python_decode"]["scaled_s"] * 1e3 / o["wxf_cz_games_read"]["ms"], 1)
        print("%-8s host decode in Python: %.1f us/ply on %d games -> %.1f s for all %d plies; cz_games_read / cz_games_replay = %.3f"
              % (level, o["host_python_decode"]["us_per_ply"], len(pick), o["host_python_decode"]["scaled_s"], plies, o["read_vs_replay"]))
        out[level] = o
    print(json.dumps(out), flush=True)


def tablebase_leg(sig):
    """The build of one table, pass by pass (host clock around a pass and the read of its counter, which synchronises), then the
    fused pass against the composed one on two snapshots: device events, one warm-up each, the two forms alternating."""
    import json
    from cchess_zero_amd._lib import TB_ILLEGAL, TB_UNKNOWN
    from cchess_zero_amd.tablebase import Tablebase, closure, entries
    tb = Tablebase(rules)
    t0 = time.perf_counter()
    for s in closure(sig):
        if s != sig:
            tb.build_one(s)
    sub_s = time.perf_counter() - t0
    n = entries(sig)[0]
    passes, stamp = [], [0.0, 0]

    def before(_, d, table):
        stamp[1] = int((table == TB_UNKNOWN).sum())
        stamp[0] = time.perf_counter()

    def after(_, d, got):
        ms = (time.perf_counter() - stamp[0]) * 1e3
        passes.append(dict(d=d, ms=round(ms, 4), undecided=stamp[1], decided=got, entries_per_s=round(n / ms * 1e3)))

    t0 = time.perf_counter()
    stats = tb.build_one(sig, progress=after, before_pass=before)
    wall = time.perf_counter() - t0
    for p in passes:
        print("pass %3d: %9.3f ms, %10d undecided before it, %9d decided = %.2f G entries/s" % (p["d"], p["ms"], p["undecided"], p["decided"], p["entries_per_s"] / 1e9))
    early, late = 1, max([p["d"] for p in passes if p["decided"]] or [1])
    final = tb.tables.pop(sig)
    snaps = {}
    tb.build_one(sig, before_pass=lambda _, d, table: snaps.__setitem__(d, table.clone()) if d in (early, late) else None)
    assert torch.equal(tb.tables[sig], final)
    subs, _ = tb.sub_tables(sig)
    work = torch.empty_like(final)
    counter = torch.zeros(1, dtype=torch.int64, device=final.device)
    big, CH = 1 << 20, 1 << 20

    def fused(d):
        ctx.call("cz_tb_pass", sig.encode(), work, subs, d, counter)

    def composed(d):
        snap = tb.tables[sig]
        out = snap.clone()
        unk = (snap == TB_UNKNOWN).nonzero().flatten().to(torch.int32)
        children = 0
        for lo in range(0, unk.numel(), CH):
            idx = unk[lo:lo + CH]
            b, sd = tb.boards(sig, idx)
            mv, cnt, _, _ = rules.movegen_kingsafe(b, sd, want_mask=False, pad=False)
            cb, cs, _, par, _ = rules.successors(b, sd, mv, cnt)
            children += cb.shape[0]
            u = tb.probe(cb, cs)[0].to(torch.int64)
            par, pl = par.to(torch.int64), u.abs() - 1
            settled = (u != TB_UNKNOWN) & (u != TB_ILLEGAL) & (pl < d)
            m = idx.numel()
            lost = torch.full((m,), big, dtype=torch.int64, device=u.device).scatter_reduce_(0, par, torch.where(settled & (u < 0), pl, big), "amin")
            all_won = torch.ones(m, dtype=torch.int64, device=u.device).scatter_reduce_(0, par, (settled & (u > 0)).to(torch.int64), "amin")
            won = torch.full((m,), -1, dtype=torch.int64, device=u.device).scatter_reduce_(0, par, torch.where(u > 0, pl, -1), "amax")
            v = torch.where(lost < big, lost + 2, torch.where(all_won == 1, -(won + 2), torch.full_like(lost, TB_UNKNOWN)))
            out[idx.to(torch.int64)] = v.to(torch.int16)
        return out, children

    out = dict(signature=sig, entries=n, sub_tables_s=round(sub_s, 4), build_s=round(wall, 4), passes=stats["passes"], stats=stats, per_pass=passes)
    for name, d in (("early", early), ("late", late)):
        snap = snaps[d]
        tb.tables[sig] = snap
        work.copy_(snap)
        fused(d)
        want, children = composed(d)                      # the warm-up of both, and the check that they compute the same pass
        assert torch.equal(work, want), "the fused and the composed pass %d differ" % d
        tf, tc = [], []
        for _ in range(3):
            work.copy_(snap)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            fused(d)
            e1.record()
            composed(d)
            e2.record()
            e2.synchronize()
            tf.append(e0.elapsed_time(e1))
            tc.append(e1.elapsed_time(e2))
        tf.sort(), tc.sort()
        undecided = int((snap == TB_UNKNOWN).sum())
        out[name] = dict(d=d, undecided=undecided, children=children, fused_ms=round(tf[1], 4), fused_min_ms=round(tf[0], 4), fused_max_ms=round(tf[2], 4),
                         composed_ms=round(tc[1], 4), composed_min_ms=round(tc[0], 4), composed_max_ms=round(tc[2], 4), composed_over_fused=round(tc[1] / tf[1], 2),
                         fused_entries_per_s=round(n / tf[1] * 1e3))
        print("%s pass %d (%d of %d undecided, %d children): fused %.3f ms (min %.3f, max %.3f), composed %.3f ms (min %.3f, max %.3f) = %.1f x"
              % (name, d, undecided, n, children, tf[1], tf[0], tf[2], tc[1], tc[0], tc[2], tc[1] / tf[1]))
    tb.tables[sig] = final
    print(json.dumps(out), flush=True)


def tablebase_set_leg(sig, n=65536, roots=8192):
    """Tablebase.probe against Tablebase.probe_set on one mixed batch, and the set's launch on a batch of misses"""
    import json
    from cchess_zero_amd._lib import TB_ILLEGAL
    from cchess_zero_amd.rules import START_BOARD
    from cchess_zero_amd.tablebase import Tablebase
    tb = Tablebase(rules)
    tb.build(sig)
    sigs = sorted(tb.tables)
    gen = torch.Generator(device=tb.dev).manual_seed(1)
    per = (n + len(sigs) - 1) // len(sigs)
    bs, ss = [], []
    for s in sigs:
        legal = (tb.tables[s] != TB_ILLEGAL).nonzero().flatten()
        idx = legal[torch.randint(0, legal.numel(), (per,), generator=gen, device=tb.dev)].to(torch.int32)
        b, sd = tb.boards(s, idx)
        bs.append(b), ss.append(sd)
    perm = torch.randperm(per * len(sigs), generator=gen, device=tb.dev)[:n]
    boards, side = torch.cat(bs)[perm].contiguous(), torch.cat(ss)[perm].contiguous()

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out
    _, ref = events(lambda: tb.probe(boards, side))                    # the warm-up of both, and the comparison
    _, got = events(lambda: tb.probe_set(boards, side))
    equal = bool(torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]))
    tp, ts = [], []
    for _ in range(3):
        tp.append(events(lambda: tb.probe(boards, side))[0])
        ts.append(events(lambda: tb.probe_set(boards, side))[0])
    tp.sort(), ts.sort()
    miss = torch.from_numpy(np.tile(np.asarray(START_BOARD, np.uint8).reshape(1, 90), (roots, 1))).to(tb.dev)
    mside = torch.zeros(roots, dtype=torch.uint8, device=tb.dev)
    tb.probe_set(miss, mside)
    tm = sorted(events(lambda: tb.probe_set(miss, mside))[0] for _ in range(5))
    all_miss = bool((tb.probe_set(miss, mside)[1] == 0).all())
    out = dict(signature=sig, tables=len(sigs), positions=n, equal=equal, probe_ms=round(tp[1], 4), probe_min_ms=round(tp[0], 4), probe_max_ms=round(tp[2], 4),
               probe_set_ms=round(ts[1], 4), probe_set_min_ms=round(ts[0], 4), probe_set_max_ms=round(ts[2], 4), probe_over_probe_set=round(tp[1] / ts[1], 2),
               roots=roots, roots_all_miss=all_miss, roots_ms=round(tm[2], 4), roots_min_ms=round(tm[0], 4), roots_max_ms=round(tm[4], 4))
    print("%d positions of %d tables: Tablebase.probe %.3f ms (min %.3f, max %.3f), probe_set %.3f ms (min %.3f, max %.3f) = %.1f x, answers %s"
          % (n, len(sigs), tp[1], tp[0], tp[2], ts[1], ts[0], ts[2], tp[1] / ts[1], "equal" if equal else "DIFFER"))
    print("%d start positions, all misses: %.4f ms per launch with its two output tensors (min %.4f, max %.4f)" % (roots, tm[2], tm[0], tm[4]))
    print(json.dumps(out), flush=True)
    assert equal and all_miss


def book_leg(n_keys=1 << 20, n_probe=1 << 16, n_games=1 << 16, launches=20):
    """the book's fused kernels against their compositions, alternating in one run, and Book.build end to end"""
    import json
    from cchess_zero_amd import games as GA
    from cchess_zero_amd.book import Book
    from cchess_zero_amd.rules import random_positions
    SIGN = -(1 << 63)
    boards, side, _ = random_positions(rules, n_keys, seed=17)
    bk = Book(ctx)

    def fused_keys(b, s):
        key = torch.empty(b.shape[0], dtype=torch.int64, device=b.device)
        mir = torch.empty(b.shape[0], dtype=torch.uint8, device=b.device)
        ctx.call("cz_book_keys", b, s, b.shape[0], key, mir)
        return key, mir

    def composed_keys(b, s):
        k = rules.hash(b, s) ^ SIGN
        km = rules.hash(b.view(-1, 10, 9).flip(2).reshape(-1, 90).contiguous(), s) ^ SIGN
        return torch.minimum(k, km) ^ SIGN, (km < k).to(torch.uint8) + 2 * (km == k).to(torch.uint8)

    def alternate(a, b):
        """(median, min, max) ms of each form over `launches` alternating calls, after one warm-up call of each"""
        a(), b()
        torch.cuda.synchronize()
        ta, tb = [], []
        for _ in range(launches):
            for fn, ts in ((a, ta), (b, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
        ta.sort(), tb.sort()
        return (ta[len(ta) // 2], ta[0], ta[-1]), (tb[len(tb) // 2], tb[0], tb[-1])
    out = dict(key_positions=n_keys)
    fk, ck = fused_keys(boards, side), composed_keys(boards, side)
    out["keys_equal"] = bool(torch.equal(fk[0], ck[0]) and torch.equal(fk[1], ck[1]))
    f, c = alternate(lambda: fused_keys(boards, side), lambda: composed_keys(boards, side))
    out.update(keys_fused_ms=[round(x, 4) for x in f], keys_composed_ms=[round(x, 4) for x in c], keys_composed_over_fused=round(c[0] / f[0], 2))
    print("cz_book_keys, %d positions: fused %.3f ms (min %.3f, max %.3f) = %.2f G positions/s; composed %.3f ms (min %.3f, max %.3f) = %.2f x; answers %s"
          % (n_keys, f[0], f[1], f[2], n_keys / f[0] / 1e6, c[0], c[1], c[2], c[0] / f[0], "equal" if out["keys_equal"] else "DIFFER"))
    # a book of the distinct keys of the 1 M positions; the probed positions: half of them from it, half from another seed
    skey = torch.unique(fk[0] ^ SIGN)          # sorted as unsigned
    bkey = (skey ^ SIGN).contiguous()
    E = int(bkey.numel())
    ob, os_, _ = random_positions(rules, n_probe // 2, seed=18)
    pb, ps = torch.cat([boards[:n_probe // 2], ob]).contiguous(), torch.cat([side[:n_probe // 2], os_]).contiguous()

    def fused_probe():
        first = torch.empty(n_probe, dtype=torch.int32, device=pb.device)
        count = torch.empty(n_probe, dtype=torch.int32, device=pb.device)
        mir = torch.empty(n_probe, dtype=torch.uint8, device=pb.device)
        ctx.call("cz_book_probe", E, bkey, pb, ps, n_probe, first, count, mir)
        return first, count, mir

    def composed_probe():
        key, mir = composed_keys(pb, ps)
        lo = torch.searchsorted(skey, key ^ SIGN, right=False)
        count = (torch.searchsorted(skey, key ^ SIGN, right=True) - lo).to(torch.int32)
        return torch.where(count > 0, lo.to(torch.int32), torch.full_like(count, -1)), count, mir
    fp, cp = fused_probe(), composed_probe()
    out.update(book_entries=E, probe_positions=n_probe, probe_hits=int((fp[0] >= 0).sum()), probe_equal=bool(all(torch.equal(x, y) for x, y in zip(fp, cp))))
    f, c = alternate(fused_probe, composed_probe)
    out.update(probe_fused_ms=[round(x, 4) for x in f], probe_composed_ms=[round(x, 4) for x in c], probe_composed_over_fused=round(c[0] / f[0], 2))
    print("cz_book_probe, %d positions (%d hits) against %d entries: fused %.3f ms (min %.3f, max %.3f); composed %.3f ms (min %.3f, max %.3f) = %.2f x; answers %s"
          % (n_probe, out["probe_hits"], E, f[0], f[1], f[2], c[0], c[1], c[2], c[0] / f[0], "equal" if out["probe_equal"] else "DIFFER"))
    # Book.build, end to end, on the records of random games
    rg = GA.random_games("xiangqi", n_games, 3, 40, engine_rules=rules)
    gs = GA.games_from_labels(rg["moves"], rg["lens"], np.random.default_rng(3).integers(-1, 2, n_games))
    rec = GA.GameReplayer(ctx).replay(gs, rules="xiangqi").records
    bk.build(rec, 40)
    torch.cuda.synchronize()
    tb, te = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        bk.build(rec, 40)
        tb.append((time.perf_counter() - t0) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        bk.entries(rec, 40)
        e1.record()
        e1.synchronize()
        te.append(e0.elapsed_time(e1))
    tb.sort(), te.sort()
    out.update(build_games=n_games, build_records=int(rec.shape[0]), build_entries=len(bk), build_ms=[round(x, 2) for x in (tb[1], tb[0], tb[2])],
               entries_launch_ms=[round(x, 4) for x in (te[1], te[0], te[2])])
    print("Book.build, %d games = %d records -> %d entries: %.1f ms end to end (min %.1f, max %.1f), of which the cz_book_entries launch %.3f ms (min %.3f, max %.3f)"
          % (n_games, rec.shape[0], len(bk), tb[1], tb[0], tb[2], te[1], te[0], te[2]))
    print(json.dumps(out), flush=True)
    assert out["keys_equal"] and out["probe_equal"]


def repetition_moves_leg(plies_before=24, record=41, fold=3, shuffle=0):
    """N games of uniform random king-safe moves from the start position (a side without one stands still): the position after
    plies_before + record - 1 plies with the record - 1 positions before it as its record.  shuffle: in the last `shuffle` plies a
    side takes back its last move whenever that is king-safe, so that positions repeat."""
    import json
    from cchess_zero_amd._lib import REP_BLACK_LOSES, REP_NONE, REP_RED_LOSES, tables
    from cchess_zero_amd.rules import START_BOARD
    dev = rules.dev
    gen = torch.Generator(device=dev).manual_seed(29)
    t = tables()
    sd = t["srcdst"].astype(np.int64)
    back = torch.from_numpy(t["lut"][sd >> 8, sd & 0xFF].astype(np.int16)).to(dev)        # the label of the move back
    last = [torch.full((N,), -1, dtype=torch.int16, device=dev) for _ in range(2)]       # the moves of the last two plies
    b = torch.from_numpy(np.tile(START_BOARD, (N, 1))).to(dev)
    s = torch.zeros(N, dtype=torch.uint8, device=dev)
    rr = torch.zeros(N, dtype=torch.int32, device=dev)
    hist_b, hist_s = [], []
    for ply in range(plies_before + record):
        if ply >= plies_before:
            hist_b.append(b.clone()); hist_s.append(s.clone())
        if ply == plies_before + record - 1:
            break
        mv, cnt, _, _ = rules.movegen_kingsafe(b, s, want_mask=False)
        c = cnt.to(torch.int64).clamp(min=0)
        pick = mv.gather(1, (torch.rand(N, generator=gen, device=dev) * c.clamp(min=1)).to(torch.int64).clamp(max=127).unsqueeze(1)).squeeze(1)
        if ply >= plies_before + record - 1 - shuffle:
            undo = torch.where(last[0] >= 0, back[last[0].to(torch.int64).clamp(min=0)], torch.full_like(pick, -1))
            can = (undo >= 0) & ((mv == undo.unsqueeze(1)) & (torch.arange(128, device=dev).unsqueeze(0) < c.unsqueeze(1))).any(1)
            pick = torch.where(can, undo, pick)
        last = [last[1], torch.where(c > 0, pick, torch.full_like(pick, -1))]
        cap, _ = rules.apply_move(b, s, torch.where(c > 0, pick, torch.full_like(pick, -1)))
        rr = torch.where(c > 0, torch.where(cap != 0, torch.zeros_like(rr), rr + 1), rr)
    hb, hs = torch.stack(hist_b, 1).contiguous(), torch.stack(hist_s, 1).contiguous()          # [N, record, 90], [N, record]
    keys = rules.hash(hb.reshape(-1, 90), hs.reshape(-1)).reshape(N, record)
    chk = (rules.in_check(hb.reshape(-1, 90), hs.reshape(-1)) & 1).reshape(N, record)
    rec = rules.threats(hb.reshape(-1, 90), hs.reshape(-1)).reshape(N, record, 4)
    window = rr.clamp(max=record - 1)
    length = torch.full((N,), record, dtype=torch.int32, device=dev)

    def fused(n):
        return rules.repetition_moves(b[:n], s[:n], keys[:n], chk[:n], rec[:n], length[:n], window[:n], fold)

    def composed(n):
        """-> (verdict, reply_verdict != 0, losing) per child in list order, and the numbers of children and grandchildren"""
        def level(pb, ps, pk, pc, pr, plen, pwin):
            mv, cnt, _, _ = rules.movegen_kingsafe(pb, ps, want_mask=False, pad=False)
            cb, cs, cap, par, _ = rules.successors(pb, ps, mv, cnt)
            par = par.to(torch.int64)
            T = cb.shape[0]
            at = plen[par].to(torch.int64).unsqueeze(1)
            k = torch.cat([pk[par], torch.zeros((T, 1), dtype=torch.int64, device=dev)], 1).scatter_(1, at, rules.hash(cb, cs).unsqueeze(1))
            f = torch.cat([pc[par], torch.zeros((T, 1), dtype=torch.uint8, device=dev)], 1).scatter_(1, at, (rules.in_check(cb, cs) & 1).unsqueeze(1))
            r = torch.cat([pr[par], torch.zeros((T, 1, 4), dtype=torch.int64, device=dev)], 1).scatter_(1, at.unsqueeze(2).expand(T, 1, 4), rules.threats(cb, cs).unsqueeze(1))
            w = torch.where(cap != 0, torch.zeros_like(plen[par]), torch.minimum(pwin[par] + 1, plen[par]))
            v, _, cause = rules.repetition_chase(k, f, r, cs, plen[par] + 1, w, fold)
            return cb, cs, k, f, r, plen[par] + 1, w, v | (cause << 4), par
        cb, cs, k1, f1, r1, l1, w1, own, par1 = level(b[:n], s[:n], keys[:n], chk[:n], rec[:n], length[:n], window[:n])
        _, _, _, _, _, _, _, rep, par2 = level(cb, cs, k1, f1, r1, l1, w1)
        loss = torch.where(s[:n][par1] != 0, REP_BLACK_LOSES, REP_RED_LOSES).to(torch.uint8)
        hit = torch.zeros(own.shape[0], dtype=torch.int32, device=dev).index_put_((par2,), ((rep & 15) == loss[par2]).to(torch.int32), accumulate=True) > 0
        return own, hit, ((own & 15) == loss) | (((own & 15) == REP_NONE) & hit), own.shape[0], rep.shape[0]

    M = min(N, 1024)
    own, hit, losing, children, grandchildren = composed(M)
    got = fused(M)
    cnt = got["count"][:M].to(torch.int64)
    live = torch.arange(128, device=dev).unsqueeze(0) < cnt.unsqueeze(1)
    equal = bool(torch.equal(got["verdict"][:M][live], own) and torch.equal((got["reply_verdict"][:M] != 0)[live], hit))
    full = fused(N)
    torch.cuda.synchronize()
    flagged = int((((full["verdict"] & 15) != 0) | (full["reply_verdict"] != 0)).any(1).sum().item())
    removed = int((full["summary"] & 1 != 0).sum().item())
    tf, tfm, tc, tfh = [], [], [], []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fused(M)
        torch.cuda.synchronize()
        tfh.append((time.perf_counter() - t0) * 1e3)
        for n, ts in ((N, tf), (M, tfm)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fused(n)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        composed(M)
        torch.cuda.synchronize()
        tc.append((time.perf_counter() - t0) * 1e3)
    med = lambda ts: sorted(ts)[len(ts) // 2]
    out = dict(positions=N, record=record, fold=fold, shuffled_plies=shuffle, positions_with_a_verdict=flagged, positions_with_a_move_removed=removed,
               fused_ms=round(med(tf), 4), fused_positions_per_s=round(N / med(tf) * 1e3), composed_positions=M, composed_children=children,
               composed_grandchildren=grandchildren, composed_ms=round(med(tc), 3), fused_ms_on_the_composed_positions=round(med(tfm), 4),
               fused_host_clock_ms_on_the_composed_positions=round(med(tfh), 4), fused_vs_composed=round(med(tc) / med(tfh), 1), answers_equal=equal)
    print("cz_repetition_moves: %d positions with %d-position records in %.3f ms (%.0f positions/s); %d with a verdict, %d with a move removed"
          % (N, record, med(tf), N / med(tf) * 1e3, flagged, removed))
    print("the composed path on %d of them (%d children, %d grandchildren): %.2f ms; the fused call on the same: %.4f ms by the same host clock "
          "(%.4f ms by device events) = %.0f x; answers equal: %s" % (M, children, grandchildren, med(tc), med(tfh), med(tfm), med(tc) / med(tfh), equal))
    print(json.dumps(out), flush=True)
    assert equal


def avoid_step_leg(G=8192, plies=24):
    """cz_match_choose on G slots with the avoid step on against off: the same openings, a constant net and 8 playouts per move, so
    that the choose step is what the plies differ in; device events around every choose, the first two plies left out."""
    import json
    from cchess_zero_amd.arena import Match, random_openings

    def forward(planes):
        B = planes.shape[0]
        return torch.ones((B, 2086), dtype=torch.float32, device=planes.device), torch.zeros((B, 1), dtype=torch.float32, device=planes.device)
    op = random_openings(G // 2, 8, seed=3)
    out = dict(slots=G, plies=plies)
    for name, avoid in (("off", False), ("on", True)):
        m = Match((forward, 8), (forward, 8), op, slots=G, max_plies=200, seed=1, rules="xiangqi", repetition=3, chase=True, avoid_repetition=avoid)
        m.start()
        ts = []
        for ply in range(plies):
            m.search(0)
            m.search(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            m.choose()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
            m.follow()
            m.adjudicate()
        ts = sorted(ts[2:])
        out["choose_ms_" + name] = round(ts[len(ts) // 2], 4)
        if avoid:
            out["avoided"], out["forced_repetitions"] = m.avoid_stats()
        m.close()
    out["avoid_step_ms"] = round(out["choose_ms_on"] - out["choose_ms_off"], 4)
    print("cz_match_choose on %d slots, rules xiangqi, fold 3, chase: %.3f ms per ply with the avoid step, %.3f ms without (median of %d plies)"
          % (G, out["choose_ms_on"], out["choose_ms_off"], plies - 2))
    print(json.dumps(out), flush=True)


if REPMOVES:
    repetition_moves_leg()
    repetition_moves_leg(shuffle=16)
    avoid_step_leg()
    sys.exit(0)
if BOOK:
    book_leg()
    sys.exit(0)
if TABLEBASE_SET:
    tablebase_set_leg(TABLEBASE_SET)
    sys.exit(0)
if TABLEBASE:
    tablebase_leg(TABLEBASE)
    sys.exit(0)
if REPLAY or REPLAY_NOTATION:
    if REPLAY:
        replay_leg()
    notation_leg()
    sys.exit(0)
if CHECKS or MATE:
    if CHECKS:
        checks_leg()
    if MATE:
        mate_leg()
    sys.exit(0)
if SUCCESSORS:
    successors_leg()
    sys.exit(0)
if KINGSAFE:
    kingsafe_leg()
    sys.exit(0)
if THREATS:
    threats_leg()
    sys.exit(0)
b0, s0, _ = bench.synth_positions(rules, 8192, seed=5)
rep = (N + 8191) // 8192
boards = b0.repeat(rep, 1)[:N].contiguous()
side = s0.repeat(rep)[:N].contiguous()


def timed(fn, iters=5):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


t = timed(lambda: rules.movegen(boards, side, want_mask=True))
print("K1 movegen (list + mask): %.3f ms for %d positions = %.2f G positions/s, %.1f GB/s of ABI traffic (613 B/position)" % (t * 1e3, N, N / t / 1e9, N * 613 / t / 1e9))
t = timed(lambda: rules.movegen(boards, side, want_mask=True, pad=False))
print("K1 movegen (list + mask, CZ_MOVES_NO_PAD): %.3f ms = %.2f G positions/s, %.1f GB/s algorithmic (312 B/position)" % (t * 1e3, N / t / 1e9, N * 312 / t / 1e9))
t = timed(lambda: rules.movegen(boards, side, want_mask=False, pad=False))
print("K1 movegen (list only, CZ_MOVES_NO_PAD)  : %.3f ms = %.2f G positions/s" % (t * 1e3, N / t / 1e9))
t = timed(lambda: rules.movegen(boards, side, want_mask=True, want_moves=False))
print("K1 movegen (mask only)  : %.3f ms = %.2f G positions/s, %.1f GB/s of ABI traffic (357 B/position), %.1f GB/s algorithmic (312 B)" % (t * 1e3, N / t / 1e9, N * 357 / t / 1e9, N * 312 / t / 1e9))
t = timed(lambda: rules.movegen(boards, side, want_mask=False))
print("K1 movegen (list only)  : %.3f ms = %.2f G positions/s, %.1f GB/s (349 B/position)" % (t * 1e3, N / t / 1e9, N * 349 / t / 1e9))
t = timed(lambda: rules.encode_planes(boards, side, torch.bfloat16, 16))
print("K3 planes (bf16 x16)    : %.3f ms = %.2f G positions/s, %.1f GB/s (2971 B/position)" % (t * 1e3, N / t / 1e9, N * 2971 / t / 1e9))
t = timed(lambda: rules.hash(boards, side))
print("Zobrist hash            : %.3f ms = %.2f G positions/s" % (t * 1e3, N / t / 1e9))
mv, cnt, _ = rules.movegen(boards, side, want_mask=False)
labels = mv[:, 0].contiguous()          # the first legal move of every position (0xFFFF where there is none: left alone)
b2, s2 = boards.clone(), side.clone()
h2 = rules.hash(b2, s2)
t = timed(lambda: rules.apply_move(b2, s2, labels, h2))
print("K2 apply_move (+ hash, capture, terminal flags): %.3f ms = %.2f G positions/s" % (t * 1e3, N / t / 1e9))
