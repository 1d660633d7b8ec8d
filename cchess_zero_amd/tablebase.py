"""Endgame tablebases under Xiangqi rules: the exact value of every position of a material class, and the move to play.

    python -m cchess_zero_amd.tablebase --build KR-KAA --dir TB
    python -m cchess_zero_amd.tablebase --probe --fen "<fen>" [--fen "<fen>" ...] [--fen-file F] --dir TB [--notation iccs|wxf|chinese]
    python -m cchess_zero_amd.tablebase --stats --dir TB
    python -m cchess_zero_amd.tablebase --longest --dir TB

prints one JSON object per line: --build and --stats one per table (signature, entries, legal, wins, losses, draws, longest_win,
longest_loss in plies, passes, seconds), --probe one per position (fen, signature, wdl "win" / "loss" / "draw" from the mover's
view — null for a position no loaded table covers —, plies, best, pv), --longest one per table (the position with the longest
win as a FEN, its plies and its line).

A table is built by retrograde analysis on the GPU (include/cchess_hip.h: TABLEBASES; cz_tb_pass, one launch per pass, in
place) after the tables of every signature a capture leads to.  A value is from the side to move's view: 0 a draw, v > 0 the
mover mates in v - 1 plies, v < 0 it is mated in -v - 1 plies; TB_ILLEGAL marks an index without a position.  Repetition,
perpetual check and chase, and any move limit are NOT part of a table — the stance of Rules.mate: a forced mate is a mate."""
import argparse
import ctypes as C
import json
import os
import time

import numpy as np
import torch

from ._lib import NSQ, TB_ILLEGAL, TB_MAX_SLOTS, TB_MISS, TB_SET_MAX, TB_UNKNOWN, call, lib
from .notation import fen_to_position, line_text, move_text, position_to_fen

FORMAT_VERSION = 1
LETTERS = "KRNCPAB"
_CODE = {"K": 1, "A": 2, "R": 3, "B": 4, "N": 5, "P": 6, "C": 7}   # red piece codes; black: + 7
STAT_KEYS = ("entries", "legal", "wins", "losses", "draws", "longest_win", "longest_loss", "passes", "seconds")


def entries(signature):
    """(entries, slots) of a signature (cz_tb_entries); ValueError for a string that is none"""
    n, s = C.c_longlong(), C.c_int()
    try:
        call("cz_tb_entries", str(signature).encode(), C.byref(n), C.byref(s))
    except Exception as e:
        raise ValueError(str(e))
    return int(n.value), int(s.value)


def slot_letters(signature):
    return signature.replace("-", "")


def sub_signature(signature, slot):
    """The signature without the letter of slot `slot` (never a king): the table a capture of that piece leads to"""
    at = slot if slot < signature.index("-") else slot + 1
    return signature[:at] + signature[at + 1:]


def closure(signature):
    """signature and every signature it reaches by dropping non-king letters, smallest first (ties by name)"""
    seen, todo = set(), [signature]
    while todo:
        s = todo.pop()
        if s not in seen:
            seen.add(s)
            todo += [sub_signature(s, i) for i, c in enumerate(slot_letters(s)) if c != "K"]
    return sorted(seen, key=lambda s: (entries(s)[0], s))


def signature_of_counts(counts):
    """counts[code], code 0 .. 14: how many squares hold the code -> the signature string, or None when there is none"""
    halves = []
    for black in (0, 1):
        if int(counts[1 + 7 * black]) != 1:
            return None
        halves.append("".join(c * int(counts[_CODE[c] + 7 * black]) for c in LETTERS))
    return "-".join(halves)


def wdl_of(v):
    """A table value -> ("win" | "loss" | "draw", plies or None); (None, None) for TB_MISS / TB_ILLEGAL"""
    v = int(v)
    if v in (TB_MISS, TB_ILLEGAL, TB_UNKNOWN):
        return None, None
    return ("draw", None) if v == 0 else ("win", v - 1) if v > 0 else ("loss", -v - 1)


class DeviceSet:
    """A cz_tb_set over loaded tables: the handle cz_tb_set_probe, cz_selfplay_set_tablebase and cz_match_set_tablebase take.
    signatures: the order `which` counts in.  It keeps the tables' tensors alive and is closed explicitly — after every self-play
    context and match it was attached to has let go of it (cz_tb_set_destroy refuses otherwise: CchessHipError)."""

    def __init__(self, ctx, tables, signatures):
        self.signatures = tuple(signatures)
        if not 1 <= len(self.signatures) <= TB_SET_MAX:
            raise ValueError("a table set holds 1 .. %d signatures, not %d" % (TB_SET_MAX, len(self.signatures)))
        self.tensors = [tables[s] for s in self.signatures]   # KeyError: a signature that is not loaded
        names = (C.c_char_p * len(self.signatures))(*[s.encode() for s in self.signatures])
        ptrs = (C.c_void_p * len(self.signatures))(*[t.data_ptr() for t in self.tensors])
        self.h = C.c_void_p()
        ctx.call("cz_tb_set_create", len(self.signatures), names, ptrs, C.byref(self.h))

    def close(self):
        if getattr(self, "h", None):
            call("cz_tb_set_destroy", self.h)
            self.h, self.tensors = None, []

    def __del__(self):   # a set still attached somewhere is left to the process' end rather than torn from under a kernel
        if getattr(self, "h", None):
            lib().cz_tb_set_destroy(self.h)


class Tablebase:
    """The loaded tables, on the device: {signature: int16 tensor [entries]}, built here (build) or read from a directory (load)."""

    def __init__(self, rules=None):
        if rules is None:
            from .rules import Rules
            rules = Rules()
        self.rules, self.ctx, self.dev = rules, rules.ctx, rules.dev
        self.tables, self.stats = {}, {}

    # ---- building -------------------------------------------------------------------------------------------------------------
    def _stats_of(self, signature, passes, seconds):
        v = self.tables[signature].to(torch.int32)
        legal = v != TB_ILLEGAL
        win, loss = legal & (v > 0), legal & (v < 0)
        return dict(entries=int(v.numel()), legal=int(legal.sum()), wins=int(win.sum()), losses=int(loss.sum()), draws=int((legal & (v == 0)).sum()),
                    longest_win=int(v[win].max()) - 1 if bool(win.any()) else -1, longest_loss=-int(v[loss].min()) - 1 if bool(loss.any()) else -1,
                    passes=int(passes), seconds=round(float(seconds), 6))

    def sub_tables(self, signature):
        """-> (cz_tb_pass's host array of device pointers: per slot the loaded table of the signature without it, NULL for a
        king; S: the largest plies in any of them, -1 if none is decided).  KeyError for a sub-signature that is not loaded."""
        subs = (C.c_void_p * entries(signature)[1])()
        S = -1
        for i, c in enumerate(slot_letters(signature)):
            if c != "K":
                s = sub_signature(signature, i)
                subs[i] = self.tables[s].data_ptr()
                S = max(S, self.stats[s]["longest_win"], self.stats[s]["longest_loss"])
        return subs, S

    def build_one(self, signature, progress=None, before_pass=None):
        """One table from the loaded tables of its sub-signatures (KeyError without one) -> its statistics.
        before_pass(signature, pass, table) is called in front of every pass >= 1 (a benchmark takes its snapshots there)."""
        n = entries(signature)[0]
        subs, S = self.sub_tables(signature)
        start = time.perf_counter()
        table = torch.empty(n, dtype=torch.int16, device=self.dev)
        decided = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.ctx.call("cz_tb_pass", signature.encode(), table, None, 0, decided)
        d = 0
        while True:   # the stop rule of include/cchess_hip.h: the first pass that decides nothing AND has d >= S + 1
            d += 1
            if before_pass:
                before_pass(signature, d, table)
            decided.zero_()
            self.ctx.call("cz_tb_pass", signature.encode(), table, subs, d, decided)
            got = int(decided.item())
            if progress:
                progress(signature, d, got)
            if got == 0 and d >= S + 1:
                break
        table[table == TB_UNKNOWN] = 0
        self.tables[signature] = table
        self.stats[signature] = self._stats_of(signature, d, time.perf_counter() - start)
        return self.stats[signature]

    def build(self, signature, progress=None):
        """The tables of signature's closure that are not loaded yet, smallest first -> {signature: statistics} of the whole
        closure.  progress(signature, pass, decided) is called after every pass."""
        entries(signature)
        out = {}
        for s in closure(signature):
            if s not in self.tables:
                self.build_one(s, progress)
            out[s] = self.stats[s]
        return out

    # ---- files ----------------------------------------------------------------------------------------------------------------
    def save(self, directory):
        """One <signature>.npz per loaded table: the int16 values, the signature string, the format version, the statistics"""
        os.makedirs(directory, exist_ok=True)
        for s, t in self.tables.items():
            np.savez_compressed(os.path.join(directory, s + ".npz"), values=t.cpu().numpy(), signature=np.array(s), version=np.int32(FORMAT_VERSION),
                                stats=np.array(json.dumps(self.stats[s])))

    def load(self, directory, signatures=None):
        """The tables of a directory (all of them, or the signatures given) -> the signatures loaded"""
        names = sorted(f[:-4] for f in os.listdir(directory) if f.endswith(".npz")) if signatures is None else list(signatures)
        for s in names:
            z = np.load(os.path.join(directory, s + ".npz"))
            if int(z["version"]) != FORMAT_VERSION or str(z["signature"]) != s:
                raise ValueError("%s: not a tablebase file of format %d for %s" % (os.path.join(directory, s + ".npz"), FORMAT_VERSION, s))
            values = np.ascontiguousarray(z["values"], np.int16)
            if values.shape != (entries(s)[0],):
                raise ValueError("%s: %d values, the signature has %d entries" % (s, values.size, entries(s)[0]))
            self.tables[s] = torch.from_numpy(values).to(self.dev)
            self.stats[s] = json.loads(str(z["stats"])) if "stats" in z.files else self._stats_of(s, 0, 0.0)
        return names

    # ---- positions ------------------------------------------------------------------------------------------------------------
    def boards(self, signature, index):
        """The positions of indices (cz_tb_boards) -> (boards u8 [G, 90], side u8 [G]) on the device; an index whose slots overlap
        gives an empty board.  ValueError for an index outside 0 .. entries - 1."""
        index = self.ctx.tensor(index, torch.int32).reshape(-1)
        G = index.shape[0]
        n = entries(signature)[0]
        if G and (int(index.min()) < 0 or int(index.max()) >= n):
            raise ValueError("Tablebase.boards: an index outside 0 .. %d" % (n - 1))
        boards = torch.empty((G, NSQ), dtype=torch.uint8, device=self.dev)
        side = torch.empty(G, dtype=torch.uint8, device=self.dev)
        self.ctx.call("cz_tb_boards", signature.encode(), index, G, boards, side)
        return boards, side

    def signatures_of(self, boards):
        """-> (the signature strings present, None for a multiset that has none; group [G] i64: which of them a board has).  The
        bincount of every board's codes, as one key per board: three bits per code 1 .. 14 (a count above 6 reads 7, which no
        signature has) and one bit for a byte that is no piece code at all."""
        key = (boards > 14).any(1).to(torch.int64) << 45
        for c in range(1, 15):
            key += (boards == c).sum(1, dtype=torch.int64).clamp(max=7) << (3 * c)
        keys, group = torch.unique(key, return_inverse=True)
        sigs = []
        for k in keys.cpu().numpy():
            counts = [0] + [(int(k) >> (3 * c)) & 7 for c in range(1, 15)]
            sigs.append(None if int(k) >> 45 else signature_of_counts(counts))
        return sigs, group

    def probe_one(self, signature, boards, side, want_index=False):
        """cz_tb_probe on one loaded table -> value i16 [G] (and index i32 [G])"""
        G = boards.shape[0]
        value = torch.empty(G, dtype=torch.int16, device=self.dev)
        index = torch.empty(G, dtype=torch.int32, device=self.dev) if want_index else None
        self.ctx.call("cz_tb_probe", signature.encode(), self.tables[signature], boards, side, G, value, index)
        return (value, index) if want_index else value

    def probe(self, boards, side):
        """The values of G positions -> (value i16 [G], covered bool [G]) on the device: the positions are grouped by their
        pieces, one cz_tb_probe per signature present; a position whose signature is not loaded answers TB_MISS.  covered: the
        value is a win, a loss or a draw (not TB_MISS, not TB_ILLEGAL)."""
        boards = self.ctx.tensor(boards, torch.uint8).reshape(-1, NSQ)
        side = self.ctx.tensor(side, torch.uint8).reshape(-1)
        value = torch.full((boards.shape[0],), TB_MISS, dtype=torch.int16, device=self.dev)
        if boards.shape[0]:
            sigs, group = self.signatures_of(boards)
            for k, s in enumerate(sigs):
                if s in self.tables:
                    at = (group == k).nonzero().flatten()
                    value[at] = self.probe_one(s, boards[at].contiguous(), side[at].contiguous())
        return value, (value != TB_MISS) & (value != TB_ILLEGAL)

    def device_set(self, signatures=None):
        """A DeviceSet over the loaded tables (all of them in sorted order, or the signatures given, in that order): one handle
        for probe_set, SelfPlay(tablebase=) and Match(tablebase=).  The caller closes it."""
        return DeviceSet(self.ctx, self.tables, sorted(self.tables) if signatures is None else list(signatures))

    def probe_set(self, boards, side, dset=None):
        """probe() in ONE launch (cz_tb_set_probe), whatever the positions' material and with no grouping on the host ->
        (value i16 [G], covered bool [G], which i32 [G]: the place of the board's signature in dset.signatures, -1 for TB_MISS).
        dset: a device_set() to probe; None: one over all loaded tables, made on first use and again when the tables change."""
        boards = self.ctx.tensor(boards, torch.uint8).reshape(-1, NSQ)
        side = self.ctx.tensor(side, torch.uint8).reshape(-1)
        if dset is None:
            have = tuple(sorted(self.tables))
            cur = getattr(self, "_set", None)
            if cur is None or cur.signatures != have or any(a is not self.tables[s] for a, s in zip(cur.tensors, have)):
                if cur is not None:
                    cur.close()
                self._set = self.device_set()
            dset = self._set
        G = boards.shape[0]
        value = torch.empty(G, dtype=torch.int16, device=self.dev)
        which = torch.empty(G, dtype=torch.int32, device=self.dev)
        self.ctx.call("cz_tb_set_probe", dset.h, boards, side, G, value, which)
        return value, (value != TB_MISS) & (value != TB_ILLEGAL), which

    def _children(self, boards, side):
        """-> (value [G], child boards, child sides, child labels, child values, parent i64 [T]): the king-safe successors of the
        covered positions, in list order"""
        value, covered = self.probe(boards, side)
        mv, cnt, _, _ = self.rules.movegen_kingsafe(boards, side, want_mask=False, pad=False)
        cnt = torch.where(covered, cnt, torch.zeros_like(cnt))
        cb, cs, _, par, label = self.rules.successors(boards, side, mv, cnt)
        return value, cb, cs, label, self.probe(cb, cs)[0], par.to(torch.int64)

    def best(self, boards, side):
        """The move to play in G positions -> (label i32 [G], value i16 [G], child boards u8 [G, 90], child sides u8 [G]) on the
        device: the FIRST king-safe move in list order whose child value is optimal — a win: the child lost in plies - 1; a loss:
        the child won in plies - 1; a draw: a child of value 0.  label -1: the position is not covered or has no king-safe move."""
        boards = self.ctx.tensor(boards, torch.uint8).reshape(-1, NSQ)
        side = self.ctx.tensor(side, torch.uint8).reshape(-1)
        G = boards.shape[0]
        value, cb, cs, label, cv, par = self._children(boards, side)
        v = value.to(torch.int32)
        want = torch.where(v > 0, 1 - v, torch.where(v < 0, -v - 1, torch.zeros_like(v)))
        T = cb.shape[0]
        first = torch.full((G,), T, dtype=torch.int64, device=self.dev)
        if T:
            hit = cv.to(torch.int32) == want[par]
            at = torch.where(hit, torch.arange(T, device=self.dev), torch.full((T,), T, dtype=torch.int64, device=self.dev))
            first.scatter_reduce_(0, par, at, "amin")
        found = first < T
        pick = first.clamp(max=max(T - 1, 0))
        out_label = torch.full((G,), -1, dtype=torch.int32, device=self.dev)
        nb, ns = boards.clone(), side.clone()
        if T:
            out_label = torch.where(found, label[pick].to(torch.int32) & 0xFFFF, out_label)
            nb = torch.where(found.unsqueeze(1), cb[pick], nb)
            ns = torch.where(found, cs[pick], ns)
        return out_label, value, nb, ns

    def line(self, board, side, max_len=512):
        """The principal line from one position, through captures into the tables of fewer pieces -> [labels]: best() ply after
        ply until a position without a king-safe move (or one that no table covers), at most max_len moves."""
        b = self.ctx.tensor(np.asarray(board, np.uint8) if not torch.is_tensor(board) else board, torch.uint8).reshape(1, NSQ)
        s = self.ctx.tensor(np.array([1 if int(side) else 0], np.uint8), torch.uint8)
        out = []
        for _ in range(int(max_len)):
            label, _, b, s = self.best(b, s)
            if int(label[0]) < 0:
                break
            out.append(int(label[0]))
        return out

    DRAW_LINE = 16

    def describe(self, board, side, notation="iccs", max_len=None):
        """What the table says about one position -> dict(wdl, plies, best, pv), moves written in `notation`; None for a position
        that no loaded table covers.  pv: the whole line to the mate, or the first max_len moves of it (a draw's line has no end:
        its first DRAW_LINE moves)"""
        board = np.asarray(board, np.uint8).reshape(NSQ)
        value, covered = self.probe(board.reshape(1, NSQ), np.array([1 if side else 0], np.uint8))
        if not bool(covered[0]):
            return None
        wdl, plies = wdl_of(int(value[0]))
        pv = self.line(board, side, (self.DRAW_LINE if plies is None else plies) if max_len is None else max_len)
        return dict(wdl=wdl, plies=plies, best=(move_text(board, side, pv[0], notation) or move_text(board, side, pv[0])) if pv else None,
                    pv=line_text(board, side, pv, notation))

    def longest(self, signature):
        """The position with the longest win of a table (the lowest such index) -> dict(fen, plies, pv), None without a win"""
        win = self.tables[signature].to(torch.int32)   # TB_ILLEGAL is negative: the maximum is the longest win
        if int(win.max()) <= 0:
            return None
        i = int(win.argmax())
        b, s = self.boards(signature, [i])
        board, sd = b[0].cpu().numpy(), int(s[0])
        return dict(fen=position_to_fen(board, sd), index=i, plies=int(win[i]) - 1, pv=line_text(board, sd, self.line(board, sd)))


def main(argv=None, tb=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.tablebase",
                                 description="Xiangqi endgame tablebases on the GPU: build, probe, statistics; one JSON object per line.")
    ap.add_argument("--build", metavar="SIG", default=None, help="build the table of a signature such as KR-KAA (and of every signature a capture leads to)")
    ap.add_argument("--probe", action="store_true", help="answer the positions given by --fen / --fen-file from the tables in --dir")
    ap.add_argument("--stats", action="store_true", help="the statistics of every table in --dir")
    ap.add_argument("--longest", action="store_true", help="the position with the longest win of every table in --dir, as a FEN")
    ap.add_argument("--dir", default=None, help="the directory of the tables: one <signature>.npz each")
    ap.add_argument("--fen", action="append", default=[], help="a position as standard Xiangqi FEN (may be given more than once)")
    ap.add_argument("--fen-file", default=None, help="a file with one FEN per line")
    ap.add_argument("--notation", choices=("iccs", "wxf", "chinese"), default="iccs", help="how the moves of the output are written (default: ICCS)")
    args = ap.parse_args(argv)
    if sum([args.build is not None, args.probe, args.stats, args.longest]) != 1:
        ap.error("give one of --build, --probe, --stats, --longest")
    if not args.dir:
        ap.error("--dir is required")
    fens = list(args.fen)
    if args.fen_file:
        fens += [l.strip() for l in open(args.fen_file) if l.strip()]
    if args.probe and not fens:
        ap.error("no position: give --fen or --fen-file")
    if fens and not args.probe:
        ap.error("--fen / --fen-file go with --probe")
    try:
        pos = [fen_to_position(f) for f in fens]
    except ValueError as e:
        ap.error(str(e))
    if args.build is not None and not _is_signature(args.build):
        ap.error("--build: %r is no signature (red pieces, '-', black pieces; letters KRNCPAB in that order, one K first)" % (args.build,))
    if tb is None:
        tb = Tablebase()
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row, ensure_ascii=args.notation != "chinese"), flush=True)

    if args.build is not None:
        if os.path.isdir(args.dir):
            have = set(f[:-4] for f in os.listdir(args.dir) if f.endswith(".npz"))
            tb.load(args.dir, [s for s in closure_names(args.build) if s in have])
        try:
            stats = tb.build(args.build)
        except ValueError as e:
            ap.error(str(e))
        tb.save(args.dir)
        for s, st in stats.items():
            emit(dict(signature=s, **st))
        return rows
    tb.load(args.dir)
    if args.stats:
        for s in sorted(tb.stats):
            emit(dict(signature=s, **tb.stats[s]))
    elif args.longest:
        for s in sorted(tb.tables):
            emit(dict(signature=s, **(tb.longest(s) or dict(fen=None, index=None, plies=None, pv=[]))))
    else:
        for f, p in zip(fens, pos):
            d = tb.describe(p[0], p[1], args.notation)
            counts = np.bincount(np.asarray(p[0], np.uint8), minlength=15)
            emit(dict(fen=f, signature=signature_of_counts(counts), **(d or dict(wdl=None, plies=None, best=None, pv=[]))))
    return rows


def _is_signature(s):
    """The signature grammar, on the host (so that a command line is refused before anything touches a GPU)"""
    halves = str(s).split("-")
    if len(halves) != 2 or len(s) - 1 > TB_MAX_SLOTS:
        return False
    most = {"K": 1, "R": 2, "N": 2, "C": 2, "P": 5, "A": 2, "B": 2}
    for h in halves:
        if not h or h[0] != "K" or any(c not in LETTERS for c in h):
            return False
        if [LETTERS.index(c) for c in h] != sorted(LETTERS.index(c) for c in h) or any(h.count(c) > most[c] for c in LETTERS):
            return False
    return True


def closure_names(signature):
    """closure() without the library: the names only, in no particular order"""
    seen, todo = set(), [signature]
    while todo:
        s = todo.pop()
        if s not in seen:
            seen.add(s)
            todo += [sub_signature(s, i) for i, c in enumerate(slot_letters(s)) if c != "K"]
    return seen


if __name__ == "__main__":
    main()
