"""An opening book from recorded games (include/cchess_hip.h: BOOK).

A book is a table of entries (key, label) -> games, wins, draws, ascending by key (unsigned 64-bit), then by label, one entry per
pair.  key is the canonical key of a position under the left-right mirror — min(cz_hash(board), cz_hash(board with its files
reversed)) — and label the played move in that orientation (mirror[label] in a mirrored position, min(label, mirror[label]) in a
self-mirror one).  The counters are uint32 from the mover's view; the games of one position's entries sum to less than 2^32.

  Book.build / from_games   one cz_book_entries launch over packed records (GameReplayer.replay's), then sort and sum
  Book.probe / choose       cz_book_probe / cz_book_choose: a batch of positions against the book in one launch
  Book.playout              games from the start position, ply by ply through games._playout, every move sampled from the book
  merge, save, load, stats  host code on the table (no GPU needed): two books of one rules level merge by concatenate, sort, sum

  python -m cchess_zero_amd.book --build --in games.pgn [--notation any] [--rules xiangqi] [--max_ply 40] [--merge OLD.npz] --out book.npz
  python -m cchess_zero_amd.book --probe --book B.npz {--fen "<fen>" | --fen-file F} [--notation iccs|wxf|chinese] [--min_games N]
  python -m cchess_zero_amd.book --stats --book B.npz [--min_games N]

Consumers: `setoption Book` of the UCCI engine, `--book` of analysis and arena (arena.book_openings).  Out of scope: book
moves forced in self-play, move ordering inside the search, other engines' book formats, repetition verdicts on the source games.
"""
import argparse
import collections
import io
import json
import sys
import zipfile

import numpy as np

from ._lib import MASK_WORDS, NLABELS, NSQ, tables

FORMAT_VERSION = 1
RULES_LEVEL = {"capture": 0, "xiangqi": 1}
FIELDS = (("key", np.uint64), ("label", np.uint16), ("games", np.uint32), ("wins", np.uint32), ("draws", np.uint32))
META = ("version", "rules", "max_ply", "source_games", "source_plies")   # the meta record: int64 [5]
SKIPPED = 255            # cz_book_entries' outcome of a record that is no entry
GAMES_LIMIT = 1 << 32    # the games of one position's entries stay below it (cz_book_choose's exact arithmetic)

Playout = collections.namedtuple("Playout", "boards side rr labels lens")


# ---- the table on the host ------------------------------------------------------------------------------------------------
def host_key(board, side):
    """The canonical key of one position on the host (the library's Zobrist table) -> (key, mirrored 0 / 1 / 2)."""
    t = tables()
    zob, b = t["zobrist"], np.asarray(board, np.uint8).reshape(10, 9)
    out = []
    for bb in (b, b[:, ::-1]):
        c = bb.reshape(NSQ).astype(np.int64)
        c = np.where(c < 15, c, 0)
        h = np.bitwise_xor.reduce(np.where(c > 0, zob[c, np.arange(NSQ)], np.uint64(0)))
        out.append(int(h) ^ (t["zobrist_side"] if side else 0))
    k, km = out
    return min(k, km), 1 if km < k else 2 if km == k else 0


def own_label(label, mirrored):
    """A stored label in the orientation of a position with that `mirrored` value."""
    return int(tables()["mirror"][label]) if mirrored == 1 else int(label)


def reduce_entries(key, label, outcome):
    """Entry tuples (canonical key u64, canonical label u16, outcome 0 win / 1 draw / 2 loss / 255 none) -> the table's five
    arrays: sorted by (key, label), one entry per pair, the counters summed."""
    key, label, outcome = np.asarray(key, np.uint64), np.asarray(label, np.uint16), np.asarray(outcome, np.uint8)
    keep = outcome != SKIPPED
    key, label, outcome = key[keep], label[keep], outcome[keep]
    return _sum_sorted(key, label, np.ones(len(key), np.uint64), (outcome == 0).astype(np.uint64), (outcome == 1).astype(np.uint64))


def _sum_sorted(key, label, games, wins, draws):
    order = np.lexsort((label, key))
    key, label = key[order], label[order]
    if len(key) == 0:
        return tuple(np.zeros(0, dt) for _, dt in FIELDS)
    head = np.concatenate([[True], (key[1:] != key[:-1]) | (label[1:] != label[:-1])])
    at = np.nonzero(head)[0]
    sums = [np.add.reduceat(np.asarray(x, np.uint64)[order], at) for x in (games, wins, draws)]
    if any(int(s.max()) >= GAMES_LIMIT for s in sums):
        raise ValueError("Book: an entry counts 2^32 games or more")
    return (key[at], label[at]) + tuple(s.astype(np.uint32) for s in sums)


def check_table(key, label, games, wins, draws):
    """ValueError unless the arrays are a book: dtypes and lengths, ascending by (key, label) without a repeated pair, labels
    below 2086, wins + draws <= games, no entry without a game, and every position's games below 2^32."""
    arrays = (key, label, games, wins, draws)
    for (name, dt), a in zip(FIELDS, arrays):
        if not isinstance(a, np.ndarray) or a.dtype != dt or a.ndim != 1 or len(a) != len(key):
            raise ValueError("Book: %s must be a %s array as long as key" % (name, np.dtype(dt).name))
    if len(key) == 0:
        return
    same = key[1:] == key[:-1]
    if (key[1:] < key[:-1]).any() or (same & (label[1:] <= label[:-1])).any():
        raise ValueError("Book: the entries are not ascending by (key, label), or a pair is there twice")
    if int(label.max()) >= NLABELS:
        raise ValueError("Book: a label is no move")
    if (games == 0).any() or (wins.astype(np.uint64) + draws > games).any():
        raise ValueError("Book: an entry without games, or with more wins and draws than games")
    at = np.nonzero(np.concatenate([[True], ~same]))[0]
    if int(np.add.reduceat(games.astype(np.uint64), at).max()) >= GAMES_LIMIT:
        raise ValueError("Book: the entries of one position count 2^32 games or more")


class Book:
    """The table, and the launches on a Context (made at the first launch: the host code needs no GPU)."""

    def __init__(self, ctx=None, device=0):
        self._ctx, self._device = ctx, device
        self.rules, self.max_ply, self.source_games, self.source_plies = "xiangqi", 0, 0, 0
        self._set(*(np.zeros(0, dt) for _, dt in FIELDS))

    @property
    def ctx(self):
        if self._ctx is None:
            from .engine import Context
            self._ctx = Context(1, 2, self._device)
        return self._ctx

    # -- the table -------------------------------------------------------------------------------------------------------
    def _set(self, key, label, games, wins, draws):
        check_table(key, label, games, wins, draws)
        self.key, self.label, self.games, self.wins, self.draws = key, label, games, wins, draws
        self._dev = None
        return self

    def set_entries(self, key, label, outcome, rules="xiangqi", max_ply=0, source_games=0, source_plies=0):
        """The book of entry tuples (reduce_entries); the launches' answers or a model's."""
        if rules not in RULES_LEVEL:
            raise ValueError("Book: rules is 'capture' or 'xiangqi'")
        self.rules, self.max_ply, self.source_games, self.source_plies = rules, int(max_ply), int(source_games), int(source_plies)
        return self._set(*reduce_entries(key, label, outcome))

    def arrays(self):
        return self.key, self.label, self.games, self.wins, self.draws

    def __len__(self):
        return len(self.key)

    def merge(self, other):
        """-> a new Book on this one's context: the entries of both, sorted, the counters of equal pairs summed."""
        if self.rules != other.rules and len(self) and len(other):
            raise ValueError("Book.merge: a %s book and a %s book" % (self.rules, other.rules))
        out = Book(self._ctx, self._device)
        out.rules = self.rules if len(self) else other.rules
        out.max_ply = max(self.max_ply, other.max_ply) if self.max_ply and other.max_ply else 0
        out.source_games, out.source_plies = self.source_games + other.source_games, self.source_plies + other.source_plies
        return out._set(*_sum_sorted(*(np.concatenate([a, b]) for a, b in zip(self.arrays(), other.arrays()))))

    def save(self, path):
        """One .npz, the same bytes for the same book: stored members with a fixed time stamp."""
        meta = np.array([FORMAT_VERSION, RULES_LEVEL[self.rules], self.max_ply, self.source_games, self.source_plies], np.int64)
        with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
            for name, a in list(zip([f for f, _ in FIELDS], self.arrays())) + [("meta", meta)]:
                buf = io.BytesIO()
                np.lib.format.write_array(buf, np.ascontiguousarray(a), version=(1, 0))
                z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue())

    def load(self, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [n for n in [f for f, _ in FIELDS] + ["meta"] if n not in z.files]
            if missing:
                raise ValueError("Book.load: %s has no %s" % (path, ", ".join(missing)))
            meta = z["meta"]
            if meta.shape != (len(META),) or int(meta[0]) != FORMAT_VERSION or int(meta[1]) not in RULES_LEVEL.values():
                raise ValueError("Book.load: %s is no book of format %d" % (path, FORMAT_VERSION))
            arrays = [z[f] for f, _ in FIELDS]
        self.rules = [k for k, v in RULES_LEVEL.items() if v == int(meta[1])][0]
        self.max_ply, self.source_games, self.source_plies = int(meta[2]), int(meta[3]), int(meta[4])
        return self._set(*arrays)

    def entries_of(self, key):
        """the range [lo, hi) of the entries of one canonical key"""
        return int(np.searchsorted(self.key, np.uint64(key), "left")), int(np.searchsorted(self.key, np.uint64(key), "right"))

    def stats(self, min_games=1):
        """dict(positions, entries, games_at_ply0: the games that start from the opening position, deepest_line: the longest
        line from there all of whose moves have games >= min_games, as ICCS text)."""
        from .rules import START_BOARD
        t = tables()
        srcdst, names = t["srcdst"], t["labels"]
        lo, hi = self.entries_of(host_key(START_BOARD, 0)[0])
        best = {}   # (canonical key) -> the longest line from there (own-orientation labels of the first board that reached it)

        def walk(board, side, path):
            key, mir = host_key(board, side)
            if key in path:   # a repetition in the source games
                return []
            if key in best:
                line = best[key][1]
                return line if best[key][0] == mir or mir == 2 or best[key][0] == 2 else [int(t["mirror"][l]) for l in line]
            a, b = self.entries_of(key)
            line = []
            for i in range(a, b):
                if int(self.games[i]) < min_games:
                    continue
                l = own_label(self.label[i], mir)
                nb = np.array(board, np.uint8, copy=True)
                src, dst = int(srcdst[l]) & 0xFF, int(srcdst[l]) >> 8
                nb[dst], nb[src] = nb[src], 0
                rest = [l] + walk(nb, 1 - side, path | {key})
                if len(rest) > len(line):
                    line = rest
            best[key] = (mir, line)
            return line
        deepest = walk(np.asarray(START_BOARD, np.uint8), 0, frozenset())
        return dict(positions=int(len(np.unique(self.key))), entries=len(self), games_at_ply0=int(self.games[lo:hi].astype(np.uint64).sum()),
                    deepest_line=[names[l] for l in deepest], rules=self.rules, max_ply=self.max_ply, source_games=self.source_games,
                    source_plies=self.source_plies)

    # -- the launches ----------------------------------------------------------------------------------------------------
    def _device_table(self):
        import torch
        if self._dev is None:
            t = self.ctx.tensor
            self._dev = (t(self.key, torch.int64), t(self.label, torch.int16), t(self.games, torch.int32), t(self.wins, torch.int32), t(self.draws, torch.int32))
        return self._dev

    def entries(self, records, max_ply=40):
        """One cz_book_entries launch -> (key i64 (u64 bits), label i16 (u16 bits), outcome u8) device tensors, one per record."""
        import torch
        rec = self.ctx.tensor(records, torch.uint8)
        n = rec.shape[0]
        key = torch.empty(n, dtype=torch.int64, device=rec.device)
        label = torch.empty(n, dtype=torch.int16, device=rec.device)
        outcome = torch.empty(n, dtype=torch.uint8, device=rec.device)
        self.ctx.call("cz_book_entries", rec, n, int(max_ply), key, label, outcome)
        return key, label, outcome

    def build(self, records, max_ply=40, rules="xiangqi", source_games=0):
        """records: uint8 [n, 608], a device tensor or a host array -> this book, of them: one cz_book_entries launch, then the
        records that are no entry dropped, the tuples sorted by (key, label) and their segments summed (reduce_entries)."""
        key, label, outcome = self.entries(records, max_ply)
        return self.set_entries(key.cpu().numpy().view(np.uint64), label.cpu().numpy().view(np.uint16), outcome.cpu().numpy(), rules, max_ply,
                                source_games, len(outcome))

    def from_games(self, games, rules="xiangqi", max_ply=40, on_illegal="truncate"):
        """Games (games.parse_games) -> this book, through GameReplayer.replay on the same context; .replay_counts: its counts."""
        from .games import GameReplayer
        r = GameReplayer(ctx=self.ctx).replay(games, rules=rules, on_illegal=on_illegal)
        self.replay_counts = r.counts
        return self.build(r.records, max_ply, rules, r.counts["kept_games"])

    def _positions(self, boards, side):
        import torch
        boards = self.ctx.tensor(boards, torch.uint8).reshape(-1, NSQ)
        return boards, self.ctx.tensor(side, torch.uint8).reshape(boards.shape[0])

    def probe_raw(self, boards, side):
        """One cz_book_probe launch -> (first i32 [G], count i32 [G], mirrored u8 [G]) device tensors."""
        import torch
        boards, side = self._positions(boards, side)
        G = boards.shape[0]
        first = torch.empty(G, dtype=torch.int32, device=boards.device)
        count = torch.empty(G, dtype=torch.int32, device=boards.device)
        mirrored = torch.empty(G, dtype=torch.uint8, device=boards.device)
        self.ctx.call("cz_book_probe", len(self), self._device_table()[0], boards, side, G, first, count, mirrored)
        return first, count, mirrored

    def probe(self, boards, side):
        """Per position the list of its book moves, dict(label (in the position's own orientation), games, wins, draws, losses,
        score = (wins + draws / 2) / games), more games first, then by label."""
        import torch
        first, count, mirrored = self.probe_raw(boards, side)
        cnt = count.to(torch.int64)
        of = torch.repeat_interleave(torch.arange(len(cnt), device=cnt.device), cnt)
        start = torch.cumsum(cnt, 0) - cnt
        idx = first.to(torch.int64)[of] + torch.arange(len(of), device=cnt.device) - start[of]
        _, dl, dg, dw, dd = self._device_table()
        lab, gm, wn, dr = (x[idx].cpu().numpy() for x in (dl, dg, dw, dd))
        lab, gm, wn, dr = lab.view(np.uint16), gm.view(np.uint32), wn.view(np.uint32), dr.view(np.uint32)
        cnt, mir = cnt.cpu().numpy(), mirrored.cpu().numpy()
        out, at = [], 0
        for g in range(len(cnt)):
            rows = []
            for i in range(at, at + int(cnt[g])):
                n, w, d = int(gm[i]), int(wn[i]), int(dr[i])
                rows.append(dict(label=own_label(lab[i], int(mir[g])), games=n, wins=w, draws=d, losses=n - w - d, score=(w + d / 2.0) / n))
            at += int(cnt[g])
            out.append(sorted(rows, key=lambda r: (-r["games"], r["label"])))
        return out

    def choose(self, boards, side, allowed=None, min_games=1, mode="most", seed=0, rnd=None):
        """One cz_book_choose launch -> (played i16 (u16 bits; -1 = 0xFFFF: nothing eligible) [G], index i32 [G]) device tensors.
        allowed: [G, 66] move sets (uint32 bits) or None; mode "most" or "sample"; seed: an int or a torch.Generator on the
        device, from which the sample's uint32 per position is drawn (rnd: those words, given)."""
        import torch
        if mode not in ("most", "sample"):
            raise ValueError("Book.choose: mode is 'most' or 'sample'")
        boards, side = self._positions(boards, side)
        G = boards.shape[0]
        if allowed is not None:
            allowed = self.ctx.tensor(allowed, torch.int32).reshape(G, MASK_WORDS)
        if mode == "sample" and rnd is None:
            gen = seed if isinstance(seed, torch.Generator) else torch.Generator(device=boards.device).manual_seed(int(seed))
            rnd = torch.randint(0, 1 << 32, (G,), generator=gen, device=boards.device, dtype=torch.int64)
        if rnd is not None:
            rnd = self.ctx.tensor(rnd, torch.int64).to(torch.int32).reshape(G)   # the low 32 bits
        played = torch.empty(G, dtype=torch.int16, device=boards.device)
        index = torch.empty(G, dtype=torch.int32, device=boards.device)
        key, label, games = self._device_table()[:3]
        self.ctx.call("cz_book_choose", len(self), key, label, games, boards, side, allowed, G, int(min_games), 1 if mode == "sample" else 0, rnd, played, index)
        return played, index

    def playout(self, n, plies, seed, min_games=1, rules="xiangqi"):
        """n games from the opening position, every move sampled from the book in proportion to its games (entries of at least
        min_games), ply by ply through games._playout under the rule level `rules`; a game that leaves the book stops there
        -> Playout(boards u8 [n, 90], side u8 [n], rr i32 [n], labels: per game the moves played, lens i32 [n]), host arrays.
        _playout plays no label that is not in the position's move list (a 64-bit key collision would end the game there)."""
        import torch
        from .games import _playout
        from .rules import START_BOARD, Rules
        if rules not in RULES_LEVEL:
            raise ValueError("Book.playout: rules is 'capture' or 'xiangqi'")
        R = Rules(ctx=self.ctx)
        dev = self.ctx.device
        gen = seed if isinstance(seed, torch.Generator) else torch.Generator(device=dev).manual_seed(int(seed))
        boards = torch.from_numpy(np.tile(START_BOARD, (int(n), 1))).to(dev)
        side = torch.zeros(int(n), dtype=torch.uint8, device=dev)
        played, lens, boards, side = _playout(R, rules, boards, side, int(plies), lambda ply, moves, count: self.choose(boards, side, None, min_games, "sample", gen)[0])
        played, lens = played.cpu().numpy().view(np.uint16), lens.cpu().numpy()
        srcdst = tables()["srcdst"]
        labels, rr = [], np.zeros(int(n), np.int32)
        for g in range(int(n)):   # the restrict round: plies since the last capture
            line = [int(x) for x in played[g, :lens[g]]]
            b = np.array(START_BOARD, np.uint8, copy=True)
            for l in line:
                src, dst = int(srcdst[l]) & 0xFF, int(srcdst[l]) >> 8
                rr[g] = 0 if b[dst] else rr[g] + 1
                b[dst], b[src] = b[src], 0
            labels.append(line)
        return Playout(boards.cpu().numpy(), side.cpu().numpy(), rr, labels, lens)


# ---- command line ---------------------------------------------------------------------------------------------------------
def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.book", description="Opening book from recorded games: build, probe, stats")
    ap.add_argument("--build", action="store_true", help="--in games -> --out book.npz")
    ap.add_argument("--probe", action="store_true", help="the book moves of --fen / --fen-file positions, one JSON object each")
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--in", dest="src", help="the games: one per line of moves, or PGN-style blocks")
    ap.add_argument("--out", help="the book written by --build")
    ap.add_argument("--merge", metavar="OLD.npz", help="--build: add the entries of this book")
    ap.add_argument("--book", metavar="B.npz", help="the book of --probe / --stats")
    ap.add_argument("--notation", default="iccs", help="--build: iccs or any (the notations read); --probe: iccs, wxf or chinese (how moves are written)")
    ap.add_argument("--rules", choices=tuple(RULES_LEVEL), default="xiangqi")
    ap.add_argument("--max_ply", type=int, default=40, help="plies of a game that enter the book (0: all)")
    ap.add_argument("--min_games", type=int, default=1, help="--probe / --stats: entries with fewer games are left out")
    ap.add_argument("--fen", action="append", default=[])
    ap.add_argument("--fen-file", default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.build + a.probe + a.stats != 1:
        ap.error("one of --build, --probe, --stats")
    if a.max_ply < 0 or a.min_games < 0:
        ap.error("--max_ply and --min_games are not negative")
    if a.build:
        from .notation import NOTATIONS
        if not a.src or not a.out:
            ap.error("--build needs --in and --out")
        if a.notation not in ("iccs", "any"):
            ap.error("--build --notation is iccs or any")
        from .games import parse_games
        old = None
        if a.merge:
            try:
                old = Book(device=a.device).load(a.merge)
            except (OSError, ValueError) as e:
                ap.error("--merge: %s" % e)
            if old.rules != a.rules:
                ap.error("--merge: %s is a %s book, --rules is %s" % (a.merge, old.rules, a.rules))
        games = parse_games(open(a.src, encoding="utf-8").read(), notations=NOTATIONS if a.notation == "any" else ("iccs",))
        book = Book(device=a.device).from_games(games, a.rules, a.max_ply)
        c = book.replay_counts
        if old is not None:
            book = old.merge(book)
        book.save(a.out)
        print(json.dumps(dict(games=c["kept_games"], plies=c["kept_plies"], entries=len(book), positions=int(len(np.unique(book.key))),
                              skipped=c["games"] - c["kept_games"] + len(games.skipped))))
        return 0
    if not a.book:
        ap.error("--probe and --stats need --book")
    try:
        book = Book(device=a.device).load(a.book)
    except (OSError, ValueError) as e:
        ap.error("--book: %s" % e)
    if a.stats:
        print(json.dumps(book.stats(a.min_games)))
        return 0
    from .notation import NOTATIONS, fen_to_position, move_text
    if a.notation not in NOTATIONS:
        ap.error("--probe --notation is one of %s" % " ".join(NOTATIONS))
    fens = list(a.fen)
    if a.fen_file:
        fens += [l.strip() for l in open(a.fen_file) if l.strip()]
    if not fens:
        ap.error("no position: give --fen or --fen-file")
    try:
        pos = [fen_to_position(f) for f in fens]
    except ValueError as e:
        ap.error(str(e))
    boards = np.stack([np.asarray(p[0], np.uint8).reshape(NSQ) for p in pos])
    side = np.array([1 if p[1] else 0 for p in pos], np.uint8)
    for f, b, s, rows in zip(fens, boards, side, book.probe(boards, side)):
        moves = [dict(r, move=move_text(b, int(s), r["label"], a.notation)) for r in rows if r["games"] >= a.min_games]
        print(json.dumps(dict(fen=f, moves=moves), ensure_ascii=a.notation != "chinese"), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
