"""The model of the endgame tablebases (TEST INFRASTRUCTURE), in Python and numpy alone, on kingsafe_model (the C oracle's
pseudo-legal generator filtered by the model's attack rule) and perft_model.make_move.  Nothing here touches cz_tablebase.h or
any kernel: cztb_rank / cztb_unrank / cztb_step, cz_tb_pass, cz_tb_probe and cz_tb_boards are held to this file bit for bit.

The definitions are those of include/cchess_hip.h (TABLEBASES), restated from its text:
    signature   "KR-KAA": red letters, '-', black letters, each side in the order KRNCPAB; every letter is a slot
    domains     K the 9 palace squares, A 5 squares, B 7, P 55, R N C all 90 (red; black: y -> 9 - y), ascending
    index       2 * mixed_radix(d0, d1, ...) + side, slot 0 the most significant digit
    value       int16 from the mover's view: 0 draw, v > 0 the mover mates in v - 1 plies, v < 0 it is mated in -v - 1 plies,
                ILLEGAL for an index without a position
A child is found by RANKING the board after the move (the k-th of equal pieces in ascending square order to their k-th
slot), not by the arithmetic on the parent's digits that the kernel does, and the passes are synchronous (every pass reads
the values of the pass before), not in place.

`PYTHONPATH=. python tests/tablebase_model.py` rewrites tests/golden/tablebase_model.npz: the tables of GOLDEN_TABLES and of
their sub-signatures (tests/test_tablebase_model_cpu.py holds the file to a fresh run of the model on the small ones)."""
import os
import sys

import numpy as np

import kingsafe_model as M
from perft_model import make_move

ILLEGAL, UNKNOWN, MISS = -32768, 32767, 32766
LETTERS = "KRNCPAB"
CODE = {"K": 1, "A": 2, "R": 3, "B": 4, "N": 5, "P": 6, "C": 7}   # red piece codes; black: + 7
MAX_COUNT = {"K": 1, "R": 2, "N": 2, "C": 2, "P": 5, "A": 2, "B": 2}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tablebase_model.npz")
GOLDEN_TABLES = ("KR-K", "KN-K", "KC-K", "KN-KA", "KN-KB", "KR-KAA", "KP-KP")   # with their closures: K-K, KP-K, K-KA, ...


def _red_domain(letter):
    if letter == "K":
        return [9 * y + x for y in range(3) for x in (3, 4, 5)]
    if letter == "A":
        return [3, 5, 13, 21, 23]
    if letter == "B":
        return [2, 6, 18, 22, 26, 38, 42]
    if letter == "P":
        return [9 * y + x for y in (3, 4) for x in (0, 2, 4, 6, 8)] + list(range(45, 90))
    return list(range(90))


def domain(letter, black):
    """The squares of a slot of this letter, ascending"""
    d = _red_domain(letter)
    if black:
        d = sorted(9 * (9 - q // 9) + q % 9 for q in d)
    return np.array(d, np.int64)


_PARSED = {}


def parse(sig):
    """-> the slots [(piece code, domain)], left to right; ValueError for a string that is no signature"""
    if sig not in _PARSED:
        _PARSED[sig] = _parse(sig)
    return _PARSED[sig]


def _parse(sig):
    halves = sig.split("-")
    if len(halves) != 2:
        raise ValueError("signature %r: red pieces, '-', black pieces" % (sig,))
    slots = []
    for black, half in enumerate(halves):
        if not half or half[0] != "K" or any(c not in LETTERS for c in half):
            raise ValueError("signature %r: every side starts with K and has letters of %s only" % (sig, LETTERS))
        if [LETTERS.index(c) for c in half] != sorted(LETTERS.index(c) for c in half) or any(half.count(c) > MAX_COUNT[c] for c in LETTERS):
            raise ValueError("signature %r: letters in the order %s, at most 1 K, 2 R N C A B, 5 P" % (sig, LETTERS))
        slots += [(CODE[c] + 7 * black, domain(c, black)) for c in half]
    return slots


def entries(sig):
    n = 2
    for _, d in parse(sig):
        n *= len(d)
    return n


def sub_signature(sig, slot):
    """The signature without the letter of slot `slot` (never a king)"""
    red = sig.index("-")
    at = slot if slot < red else slot + 1
    assert sig[at] != "K"
    return sig[:at] + sig[at + 1:]


def closure(sig):
    """sig and every signature it reaches by dropping non-king letters, smallest first (ties by name)"""
    seen, todo = set(), [sig]
    while todo:
        s = todo.pop()
        if s in seen:
            continue
        seen.add(s)
        n = len(s) - 1
        todo += [sub_signature(s, i) for i in range(n) if s.replace("-", "")[i] != "K"]
    return sorted(seen, key=lambda s: (entries(s), s))


def unrank(sig, index):
    """-> (board uint8 [90] or None when two slots share a square, side)"""
    slots = parse(sig)
    side, m = int(index) & 1, int(index) >> 1
    board = np.zeros(90, np.uint8)
    overlap = False
    for code, d in reversed(slots):
        q = d[m % len(d)]
        m //= len(d)
        overlap |= board[q] != 0
        board[q] = code
    return (None if overlap else board), side


def rank(sig, board, side):
    """-> the index of the position (the k-th of equal pieces in ascending square order on their k-th slot), None for a board
    with other pieces than the signature's or with a piece outside its domain"""
    slots = parse(sig)
    board = np.asarray(board)
    if int((board != 0).sum()) != len(slots):
        return None
    m, used = 0, {}
    for code, d in slots:
        sq = np.nonzero(board == code)[0]
        k = used.get(code, 0)
        used[code] = k + 1
        if k >= len(sq):
            return None
        at = np.nonzero(d == sq[k])[0]
        if len(at) == 0:
            return None
        m = m * len(d) + int(at[0])
    if any(int((board == code).sum()) != n for code, n in used.items()):
        return None
    return 2 * m + int(side)


def signature_of(board):
    """The signature of a board's pieces (None: no signature, e.g. a king is missing)"""
    board = np.asarray(board)
    out = []
    for black in (0, 1):
        half = "".join(c * int((board == CODE[c] + 7 * black).sum()) for c in LETTERS)
        out.append(half)
    sig = "-".join(out)
    try:
        parse(sig)
    except ValueError:
        return None
    return sig


def plies(v):
    return np.abs(np.asarray(v, np.int64)) - 1


class Table:
    """One signature's table with what the tests ask of it: values int16 [entries], passes, and the successor lists of the
    indices that were UNKNOWN after pass 0 as CSR arrays (parent, offsets, child table name index, child index, label)."""

    def __init__(self, sig, values, passes, parents, offsets, child_tab, child_idx, child_label, tabs):
        self.sig, self.values, self.passes = sig, values, passes
        self.parents, self.offsets, self.child_tab, self.child_idx, self.child_label, self.tabs = parents, offsets, child_tab, child_idx, child_label, tabs

    def stats(self):
        v = self.values.astype(np.int64)
        legal = v != ILLEGAL
        win, loss = legal & (v > 0), legal & (v < 0)
        return dict(entries=len(v), legal=int(legal.sum()), wins=int(win.sum()), losses=int(loss.sum()), draws=int((legal & (v == 0)).sum()),
                    longest_win=int(plies(v[win]).max()) if win.any() else -1, longest_loss=int(plies(v[loss]).max()) if loss.any() else -1,
                    passes=self.passes)


def build(sig, done, stop_at_first_empty_pass=False):
    """The table of sig; done: {signature: Table} of every signature a capture leads to.  stop_at_first_empty_pass: the WRONG
    stop rule, kept so that a test can show that KP-KP tells the two apart."""
    n = entries(sig)
    values = np.full(n, UNKNOWN, np.int16)
    tabs = [sig]
    parents, counts, ctab, cidx, clab = [], [], [], [], []
    for i in range(n):
        board, side = unrank(sig, i)
        if board is None:
            values[i] = ILLEGAL
            continue
        moves, flags = M.kingsafe(board, side)
        if flags & M.CAN_TAKE_KING:
            values[i] = ILLEGAL
        elif len(moves) == 0:
            values[i] = -1
        else:
            parents.append(i)
            counts.append(len(moves))
            for m in moves:
                child, cap = make_move(board, m)
                cs = sig if not cap else signature_of(child)
                if cs not in tabs:
                    tabs.append(cs)
                ctab.append(tabs.index(cs))
                cidx.append(rank(cs, child, 1 - side))
                clab.append(int(m))
    parents, ctab, cidx = np.array(parents, np.int64), np.array(ctab, np.int64), np.array(cidx, np.int64)
    offsets = np.zeros(len(parents) + 1, np.int64)
    np.cumsum(np.array(counts, np.int64), out=offsets[1:])
    # the children in other tables never change: their values once
    fixed = np.zeros(len(cidx), np.int64)
    S = -1
    for t in range(1, len(tabs)):
        sub = done[tabs[t]].values.astype(np.int64)
        fixed[ctab == t] = sub[cidx[ctab == t]]
        decided = (sub != ILLEGAL) & (sub != 0)
        if decided.any():
            S = max(S, int(plies(sub[decided]).max()))
    own = ctab == 0
    d = 0
    while len(parents):
        d += 1
        u = np.where(own, values.astype(np.int64)[np.where(own, cidx, 0)], fixed)
        settled = (u != UNKNOWN) & (u != ILLEGAL) & (plies(u) < d)
        big = 1 << 20
        seg = offsets[:-1]
        win_p = np.minimum.reduceat(np.where(settled & (u < 0), plies(u), big), seg)
        lose_ok = np.minimum.reduceat((settled & (u > 0)).astype(np.int64), seg)
        lose_p = np.maximum.reduceat(np.where(u > 0, plies(u), -1), seg)
        open_ = values[parents] == UNKNOWN
        win = open_ & (win_p < big)
        loss = open_ & ~win & (lose_ok == 1)
        values[parents[win]] = (win_p[win] + 2).astype(np.int16)
        values[parents[loss]] = (-(lose_p[loss] + 2)).astype(np.int16)
        decided = int(win.sum() + loss.sum())
        if decided == 0 and (stop_at_first_empty_pass or d >= S + 1):
            break
    values[values == UNKNOWN] = 0
    return Table(sig, values, d, parents, offsets, ctab, cidx, np.array(clab, np.uint16), tabs)


def build_closure(sig, done=None, log=None):
    """-> {signature: Table} of sig's closure (done: tables that exist already)"""
    done = {} if done is None else done
    for s in closure(sig):
        if s not in done:
            done[s] = build(s, done)
            if log:
                log("%-8s %s" % (s, done[s].stats()))
    return done


def line(tables, board, side, max_len=256):
    """The principal line from a position: at every ply the FIRST king-safe move in list order whose child value is optimal
    (win: the child lost in plies - 1; loss: the child won in plies - 1; draw: a child of value 0) -> [labels]; ends at a
    position without a king-safe move, and after max_len moves."""
    out = []
    board = np.asarray(board, np.uint8)
    for _ in range(max_len):
        sig = signature_of(board)
        v = int(tables[sig].values[rank(sig, board, side)])
        moves = M.kingsafe(board, side)[0]
        if len(moves) == 0:
            break
        want = 0 if v == 0 else (-(v - 1) if v > 0 else -v - 1)
        for m in moves:
            child = make_move(board, m)[0]
            cs = signature_of(child)
            if int(tables[cs].values[rank(cs, child, 1 - side)]) == want:
                out.append(int(m))
                board, side = child, 1 - side
                break
        else:
            raise AssertionError("no child of value %d below a position of value %d" % (want, v))
    return out


def golden():
    """{signature: int16 values} of the committed file"""
    z = np.load(GOLDEN)
    return {k.replace("_", "-"): z[k] for k in z.files if not k.startswith("passes")}, {k[7:].replace("_", "-"): int(z[k]) for k in z.files if k.startswith("passes_")}


if __name__ == "__main__":
    done = {}
    for s in (sys.argv[1:] or GOLDEN_TABLES):
        build_closure(s, done, log=lambda t: print(t, flush=True))
    out = {s.replace("-", "_"): t.values for s, t in done.items()}
    out.update({"passes_" + s.replace("-", "_"): np.int32(t.passes) for s, t in done.items()})
    if len(sys.argv) == 1:
        np.savez_compressed(GOLDEN, **out)
        print("%s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)))
