"""A UCCI engine (the protocol Xiangqi GUIs and match tools speak) on stdin / stdout.

    python -m cchess_zero_amd.ucci --model M.pt --blocks 7 [--playout 400] [--search_threads 16]

Commands: ucci, isready, setoption <name> <value> (Playouts, MultiPV, Notation, MateSearch, Tablebase, Book, BookMinGames, BookSample,
Repetition, Chase), position {startpos | fen <fen>} [moves m1 m2 ...],
banmoves m1 ..., go [nodes N | time T | depth D], stop, quit.  Moves are ICCS coordinates ("h2e2": files a-i, ranks 0-9 with
red at rank 0), positions standard Xiangqi FEN (notation.fen_to_position).  After each go: one `info depth <len> [multipv k]
score <round(1000 q)> nodes <sims> time <ms> pv m1 m2 ...` per line, then `bestmove m1 [ponder m2]`, or `nobestmove` when the
mover has no king-safe move that is not banned.  Unknown commands are ignored.  `setoption Notation wxf` (or chinese; default
iccs, which is what GUIs read) writes the pv of the info lines in that notation; bestmove and ponder stay ICCS.

`setoption MateSearch N` (N odd, 1 .. 15; default 0 = off, and nothing changes): every go first asks the searcher for a
continuous-check mate within N plies (Rules.mate, "checks" mode).  If there is one and its first move is not banned, the engine
prints `info depth <d> score <30000 - d> nodes <nodes> time <ms> pv ...` (d = the plies to the mate) and `bestmove` without
searching; otherwise it searches as without the option.  (The `ucci` banner lists Playouts and MultiPV as before.)

`setoption Tablebase <dir>` (default: unset, and nothing changes; `setoption Tablebase none` unsets it): every go first asks the
searcher for the position's value in the endgame tables of that directory (python -m cchess_zero_amd.tablebase --build).  A
covered position is answered at once, as MateSearch answers a mate: `info depth <len> score <s> nodes 0 time <ms> pv ...`, then
`bestmove` — s is 30000 - plies for a win, -30000 + plies for a loss and 0 for a draw, the pv the table's principal line.  When
banmoves bans the table's best move, or no table covers the position, the engine goes on as without the option.

`setoption Book <file>` (default: unset, and nothing changes; `setoption Book none` unsets it): every go asks the searcher for a
move from that opening book (python -m cchess_zero_amd.book --build) AFTER the tablebase and the mate solver and before the
search, among the king-safe moves that are not banned and have at least `setoption BookMinGames N` games (default 2): the most
played one, or with `setoption BookSample true` (default false) one drawn in proportion to the games.  A book move is answered
at once: `info string book games G wins W draws D losses L`, `info depth 1 score <round(1000 (2 score - 1))> nodes 0 time <ms> pv
<move>` — score = (wins + draws / 2) / games from the mover's view — and `bestmove`.  A position whose only book moves are banned,
or that is not in the book, is searched as without the option.

`setoption Repetition N` (N = 2 .. 8, 3 is the usual rule; default 0 = off, and nothing changes) and `setoption Chase true`
(default false): the engine keeps every position of the `position` command — from its start position on, the FEN's halfmove
clock and the captures saying how far back a repetition can reach — and every go first asks the searcher what the repetition
rule (with Chase: and the perpetual-chase rule) would answer after each king-safe move and after each reply to it
(Rules.repetition_moves, one launch).  A move that loses — it completes the N-th occurrence with the mover as the side that
checked or chased perpetually, or some reply to it does — is banned like a GUI's banmoves: `info string repetition: banned <moves>`.
A move after which the OPPONENT has lost by that rule is played at once, before the tablebase, the mate solver and the book:
`info string repetition: <move> ends the game, the opponent <checked|chased> perpetually`, `info depth 1 score 29999 nodes 0 time
<ms> pv <move>`, `bestmove`.  When every move loses the engine says `info string repetition: every move loses` and searches as
without the option — also when the moves that do not lose are all banned by the GUI.  The tablebase, mate and book answers
respect the ban.

The search is the one analysis.py describes: the reference's king-capture search with the Xiangqi rules applied at the root.
Out of scope: verdicts inside the tree (the search below the root does not know the repetition rule), forced sequences longer
than a move and its reply, preferring or avoiding DRAWS by repetition (Rules.repetition_moves reports them; the engine does not
act on them); the engine does not ponder (`ponder m2` is only the line's second move), and it does not reuse the tree between
position commands — every go starts from a fresh root.

UcciEngine(searcher, inp, out) is the protocol loop; `searcher` is what it needs from a search:
    set_position(board uint8[90], side, restrict round)
    kingsafe_mask() -> (uint32 [66] move set of the position, its CZ_POS_* flags)
    search(playouts) -> simulations completed by the call (the tree of the position is kept between calls)
    lines(allowed uint32 [66], n_lines, max_len) -> [dict(pv=[labels], visits=[...], q=[...])] in rank order
    width (optional attribute): simulations in flight per lock-step
    mate(plies) -> (dist, [labels], nodes) or None: a continuous-check mate of the position (only called with MateSearch > 0)
    tablebase(directory) -> (value, [labels]) or None: the position's value in the endgame tables of the directory (int16 as
        include/cchess_hip.h defines it, from the mover's view) and the table's line; None when no table covers the position
        (only called after setoption Tablebase)
    book(file, allowed uint32 [66], min_games, sample) -> (label, dict(games, wins, draws, losses, score)) or None: a move of
        the position from the opening book in that file, among `allowed` (only called after setoption Book)
    repetition_moves(boards uint8 [n, 90], sides [n], window, fold, chase) -> dict(moves, verdict, reply, reply_verdict: one
        entry per king-safe move of the LAST position, allowed uint32 [66], summary) as Rules.repetition_moves answers on the
        game whose positions these are, the last one's window being `window` (only called with Repetition > 0)
AnalyzerSearcher provides it on one device tree; the tests fake it on the C oracle.
"""
import argparse
import queue
import sys
import threading
import time

import numpy as np

from . import _lib
from .notation import NOTATIONS, START_FEN, fen_to_position, line_text

CHUNK_STEPS = 32     # lock-steps between two looks at the clock / the input
MAX_MULTIPV = 8
MAX_MATE_PLIES = 15
MATE_SCORE = 30000   # a mate in d plies scores MATE_SCORE - d
PV_LEN = 16


class UcciEngine:
    def __init__(self, searcher, inp, out, playouts=400, clock=time.monotonic):
        self.searcher, self.inp, self.out, self.clock = searcher, inp, out, clock
        self.options = dict(playouts=int(playouts), multipv=1)
        self.mate_plies = 0         # setoption MateSearch: the horizon of the mate solver in front of every go, 0 = off
        self.pv_notation = "iccs"   # setoption Notation: how the info lines write their pv
        self.tablebase_dir = None   # setoption Tablebase: the directory of the endgame tables asked in front of every go, None = off
        self.book_file, self.book_min_games, self.book_sample = None, 2, False   # setoption Book / BookMinGames / BookSample
        self.repetition, self.chase = 0, False   # setoption Repetition / Chase: the fold of the repetition rule (0 = off), the chase rule
        t = _lib.tables()
        self.labels, self.label2i, self.srcdst = t["labels"], t["label2i"], t["srcdst"]
        self.pos = fen_to_position(START_FEN)
        self.history = [self.pos]   # every position of the last position command, the start first; history[-1] is pos
        self.ban = []
        self.searcher.set_position(*self.pos)
        self._lines = queue.Queue()
        self._deferred = []

    # -- output / input ------------------------------------------------------------------------------------------------------
    def say(self, text):
        self.out.write(text + "\n")
        self.out.flush()

    def _reader(self):
        for line in self.inp:
            self._lines.put(line)
        self._lines.put(None)   # end of input: quit

    def _next(self):
        return self._deferred.pop(0) if self._deferred else self._lines.get()

    def _stop_requested(self):
        """Between two chunks of a search: `stop` ends it, `isready` is answered, everything else waits for the search's end."""
        while True:
            try:
                line = self._lines.get_nowait()
            except queue.Empty:
                return False
            word = line.split()[0] if line and line.split() else ""
            if word == "stop":
                return True
            if word == "isready":
                self.say("readyok")
            else:
                self._deferred.append(line)
                if line is None:
                    return False

    def run(self):
        threading.Thread(target=self._reader, daemon=True).start()
        while True:
            line = self._next()
            if line is None or not self.handle(line):
                break
        self.say("bye")

    # -- commands ------------------------------------------------------------------------------------------------------------
    def handle(self, line):
        """One command line -> False when it was quit."""
        tok = line.split()
        if not tok:
            return True
        cmd, args = tok[0], tok[1:]
        if cmd == "quit":
            return False
        if cmd == "ucci":
            self.say("id name cchess-zero-amd")
            self.say("id author the cchess-zero-amd authors")
            self.say("option Playouts type spin min 1 max 1000000 default %d" % self.options["playouts"])
            self.say("option MultiPV type spin min 1 max %d default 1" % MAX_MULTIPV)
            self.say("ucciok")
        elif cmd == "isready":
            self.say("readyok")
        elif cmd == "setoption":
            self.setoption(args)
        elif cmd == "position":
            self.position(args)
        elif cmd == "banmoves":
            self.banmoves(args)
        elif cmd == "go":
            self.go(args)
        return True   # stop outside a search and unknown commands: ignored

    def setoption(self, args):
        if len(args) < 2:
            return
        name = args[0].lower()
        if name == "notation":
            if args[1].lower() not in NOTATIONS:
                return self.say("info string setoption Notation: %r is not one of %s" % (args[1], " ".join(NOTATIONS)))
            self.pv_notation = args[1].lower()
            return
        if name == "tablebase":
            value = " ".join(args[1:])
            self.tablebase_dir = None if value.lower() == "none" else value
            return
        if name == "book":
            value = " ".join(args[1:])
            self.book_file = None if value.lower() == "none" else value
            return
        if name == "booksample":
            if args[1].lower() not in ("true", "false"):
                return self.say("info string setoption BookSample: %r is not true or false" % args[1])
            self.book_sample = args[1].lower() == "true"
            return
        if name == "chase":
            if args[1].lower() not in ("true", "false"):
                return self.say("info string setoption Chase: %r is not true or false" % args[1])
            self.chase = args[1].lower() == "true"
            return
        try:
            value = int(args[1])
        except ValueError:
            return self.say("info string setoption %s: %r is no number" % (args[0], args[1]))
        if name == "playouts":
            self.options["playouts"] = max(1, value)
        elif name == "multipv":
            self.options["multipv"] = min(max(1, value), MAX_MULTIPV)
        elif name == "matesearch":
            if value != 0 and (value < 1 or value > MAX_MATE_PLIES or value % 2 == 0):
                return self.say("info string setoption MateSearch: %d is not 0 (off) or an odd number of plies up to %d" % (value, MAX_MATE_PLIES))
            self.mate_plies = value
        elif name == "bookmingames":
            self.book_min_games = max(0, value)
        elif name == "repetition":
            if value != 0 and (value < 2 or value > 8):
                return self.say("info string setoption Repetition: %d is not 0 (off) or 2..8" % value)
            self.repetition = value

    def _legal(self, pos, text):
        """Is `text` a king-safe move of pos?  (The searcher is left on pos.)"""
        label = self.label2i.get(text)
        if label is None:
            return None
        self.searcher.set_position(*pos)
        mask, _ = self.searcher.kingsafe_mask()
        return label if (int(mask[label >> 5]) >> (label & 31)) & 1 else None

    def apply(self, pos, label):
        """pos after the move: the restrict round counts the plies since the last capture."""
        board, side, rr = pos
        src, dst = int(self.srcdst[label]) & 0xFF, int(self.srcdst[label]) >> 8
        nb = np.array(board, np.uint8, copy=True)
        capture = nb[dst] != 0
        nb[dst], nb[src] = nb[src], 0
        return nb, 1 - side, 0 if capture else rr + 1

    def position(self, args):
        """position {startpos | fen <fen>} [moves ...]: on a malformed FEN or an illegal move one `info string` line, and the
        previous position (with its history and its banmoves) stays."""
        moves = args[args.index("moves") + 1:] if "moves" in args else []
        head = args[:args.index("moves")] if "moves" in args else args
        try:
            if head[:1] == ["startpos"]:
                pos = fen_to_position(START_FEN)
            elif head[:1] == ["fen"]:
                pos = fen_to_position(" ".join(head[1:]))
            else:
                raise ValueError("position startpos | position fen <fen>")
            history = [pos]
            for m in moves:
                label = self._legal(pos, m)
                if label is None:
                    raise ValueError("illegal move %s in %s" % (m, " ".join(args)))
                pos = self.apply(pos, label)
                history.append(pos)
        except ValueError as e:
            self.searcher.set_position(*self.pos)
            return self.say("info string %s" % e)
        self.pos, self.history, self.ban = pos, history, []
        self.searcher.set_position(*pos)

    def banmoves(self, args):
        for m in args:
            if m in self.label2i:
                self.ban.append(self.label2i[m])
            else:
                self.say("info string banmoves: no such move %s" % m)

    def _repetition(self, s, allowed, ban):
        """In front of a go with Repetition > 0: takes the moves that lose by the repetition rule out of `allowed` and into
        `ban`, says so -> the label of an allowed move after which the opponent has lost by it, or None."""
        boards = np.stack([np.asarray(p[0], np.uint8) for p in self.history])
        sides = np.array([p[1] for p in self.history], np.uint8)
        r = s.repetition_moves(boards, sides, int(self.pos[2]), self.repetition, self.chase)
        moves, verdict = [int(m) for m in r["moves"]], [int(v) for v in r["verdict"]]
        if int(r["summary"]) & _lib.REPMOVES_FORCED:
            self.say("info string repetition: every move loses")
        else:
            kept = np.asarray(r["allowed"], np.uint32)
            lost = [m for m in moves if not (int(kept[m >> 5]) >> (m & 31)) & 1]
            if lost and not (allowed & kept).any():   # the GUI has banned every move that does not lose: a losing move is still a move
                self.say("info string repetition: every move loses")
            elif lost:
                ban.extend(lost)
                allowed &= kept
                self.say("info string repetition: banned %s" % " ".join(self.labels[m] for m in lost))
        opponent = _lib.REP_RED_LOSES if self.pos[1] else _lib.REP_BLACK_LOSES
        for m, v in zip(moves, verdict):
            if v & 15 == opponent and (int(allowed[m >> 5]) >> (m & 31)) & 1:
                self.say("info string repetition: %s ends the game, the opponent %s perpetually"
                         % (self.labels[m], "chased" if v >> 4 == _lib.CAUSE_CHASE else "checked"))
                return m
        return None

    def go(self, args):
        mode, amount = "playouts", self.options["playouts"]
        for k in ("nodes", "time", "depth"):
            if k in args[:-1]:
                try:
                    mode, amount = k, max(1, int(args[args.index(k) + 1]))
                except ValueError:
                    pass
        start = self.clock()
        s = self.searcher
        s.set_position(*self.pos)    # a fresh root for every go
        mask, _ = s.kingsafe_mask()
        allowed = np.array(mask, np.uint32)
        for label in self.ban:
            allowed[label >> 5] &= ~(np.uint32(1) << np.uint32(label & 31))
        if not allowed.any():
            return self.say("nobestmove")
        ban = list(self.ban)
        if self.repetition:
            won = self._repetition(s, allowed, ban)
            if won is not None:
                ms = int(round((self.clock() - start) * 1000.0))
                self.say("info depth 1 score %d nodes 0 time %d pv %s" % (MATE_SCORE - 1, ms, " ".join(line_text(self.pos[0], self.pos[1], [won], self.pv_notation))))
                return self.say("bestmove %s" % self.labels[won])
        if self.tablebase_dir:
            found = s.tablebase(self.tablebase_dir)
            if found is not None and found[1] and found[1][0] not in ban:
                value, pv = found
                plies = abs(int(value)) - 1
                score = 0 if value == 0 else MATE_SCORE - plies if value > 0 else plies - MATE_SCORE
                ms = int(round((self.clock() - start) * 1000.0))
                self.say("info depth %d score %d nodes 0 time %d pv %s" % (len(pv), score, ms, " ".join(line_text(self.pos[0], self.pos[1], pv, self.pv_notation))))
                return self.say("bestmove %s%s" % (self.labels[pv[0]], " ponder %s" % self.labels[pv[1]] if len(pv) > 1 else ""))
        if self.mate_plies:
            found = s.mate(self.mate_plies)
            if found is not None and found[1] and found[1][0] not in ban:
                dist, pv, nodes = found
                ms = int(round((self.clock() - start) * 1000.0))
                self.say("info depth %d score %d nodes %d time %d pv %s" % (dist, MATE_SCORE - dist, nodes, ms,
                                                                           " ".join(line_text(self.pos[0], self.pos[1], pv, self.pv_notation))))
                return self.say("bestmove %s%s" % (self.labels[pv[0]], " ponder %s" % self.labels[pv[1]] if len(pv) > 1 else ""))
        if self.book_file:
            found = s.book(self.book_file, allowed, self.book_min_games, self.book_sample)
            if found is not None:
                label, n = found
                ms = int(round((self.clock() - start) * 1000.0))
                self.say("info string book games %d wins %d draws %d losses %d" % (n["games"], n["wins"], n["draws"], n["losses"]))
                self.say("info depth 1 score %d nodes 0 time %d pv %s" % (int(round(1000.0 * (2.0 * n["score"] - 1.0))), ms,
                                                                          " ".join(line_text(self.pos[0], self.pos[1], [label], self.pv_notation))))
                return self.say("bestmove %s" % self.labels[label])
        chunk = CHUNK_STEPS * max(1, int(getattr(s, "width", 1)))
        budget = amount if mode in ("playouts", "nodes") else self.options["playouts"] if mode == "depth" else None
        sims = 0
        while True:
            n = chunk if budget is None else min(chunk, budget - sims)
            if n <= 0:
                break
            done = s.search(n)
            sims += done
            if done <= 0 or self._stop_requested():
                break
            if mode == "time" and (self.clock() - start) * 1000.0 >= 0.9 * amount:
                break
            if mode == "depth":
                top = s.lines(allowed, 1, min(max(amount, 1), 64))
                if top and len(top[0]["pv"]) >= amount:
                    break
        lines = s.lines(allowed, self.options["multipv"], min(64, max(PV_LEN, amount if mode == "depth" else 0)))
        if not lines:
            return self.say("nobestmove")
        ms = int(round((self.clock() - start) * 1000.0))
        for k, ln in enumerate(lines):
            multipv = " multipv %d" % (k + 1) if self.options["multipv"] > 1 else ""
            self.say("info depth %d%s score %d nodes %d time %d pv %s" % (len(ln["pv"]), multipv, int(round(1000.0 * float(ln["q"][0]))), sims, ms,
                                                                         " ".join(line_text(self.pos[0], self.pos[1], ln["pv"], self.pv_notation))))
        pv = lines[0]["pv"]
        self.say("bestmove %s%s" % (self.labels[pv[0]], " ponder %s" % self.labels[pv[1]] if len(pv) > 1 else ""))


class AnalyzerSearcher:
    """The searcher of UcciEngine on tree 0 of an Analyzer (games = 1, rules "xiangqi")."""

    def __init__(self, analyzer):
        assert analyzer.rules == "xiangqi", "a UCCI engine plays by the Xiangqi rules"
        self.a = analyzer
        self.width = analyzer.engine.width
        self.pos, self._rooted = None, False
        self._tb = {}   # directory -> its loaded Tablebase
        self._books = {}   # file -> its loaded Book
        self._book_seed = 0

    def set_position(self, board, side, rr):
        self.pos = (np.asarray(board, np.uint8).reshape(1, 90), np.array([1 if side else 0], np.uint8), np.array([int(rr)], np.int32))
        self._rooted = False   # the tree is reset by the first search of the position

    def kingsafe_mask(self):
        allowed, flags = self.a.root_masks(self.pos[0], self.pos[1])
        return allowed.cpu().numpy().view(np.uint32)[0], int(flags[0])

    def mate(self, plies):
        r = self.a.rule_kernels.mate(self.pos[0], self.pos[1], plies)
        if int(r["status"][0]) != 1:
            return None
        return int(r["dist"][0]), [int(l) for l in r["pv"][0] if int(l) != 0xFFFF], int(r["nodes"][0])

    def tablebase(self, directory):
        if directory not in self._tb:
            from .tablebase import Tablebase
            self._tb[directory] = Tablebase(self.a.rule_kernels)
            self._tb[directory].load(directory)
        tb = self._tb[directory]
        value, covered = tb.probe(self.pos[0], self.pos[1])
        if not bool(covered[0]):
            return None
        v = int(value[0])
        return v, tb.line(self.pos[0][0], int(self.pos[1][0]), abs(v) - 1 if v else PV_LEN)

    def book(self, file, allowed, min_games, sample):
        if file not in self._books:
            from .book import Book
            self._books[file] = Book(self.a.engine.ctx).load(file)
        bk = self._books[file]
        self._book_seed += 1   # another draw at every go
        mask = np.ascontiguousarray(allowed, np.uint32).reshape(1, -1)
        played, index = bk.choose(self.pos[0], self.pos[1], mask, min_games, "sample" if sample else "most", seed=self._book_seed)
        i = int(index[0])
        if i < 0:
            return None
        n, w, d = int(bk.games[i]), int(bk.wins[i]), int(bk.draws[i])
        return int(played[0]) & 0xFFFF, dict(games=n, wins=w, draws=d, losses=n - w - d, score=(w + d / 2.0) / n)

    def repetition_moves(self, boards, sides, window, fold, chase):
        """The history's keys, check flags and chase records in one batch each, then the fused call on the last position"""
        rk = self.a.rule_kernels
        n = len(boards)
        keys = rk.hash(boards, sides).reshape(1, n)
        checks = (rk.in_check(boards, sides) & _lib.POS_IN_CHECK).reshape(1, n)
        recs = rk.threats(boards, sides).reshape(1, n, 4) if chase else None
        r = rk.repetition_moves(boards[-1:], sides[-1:], keys, checks, recs, None, np.array([window], np.int32), fold)
        count = int(r["count"][0])
        row = lambda k, dt: r[k][0].cpu().numpy().view(dt)
        return dict(moves=row("moves", np.uint16)[:count], verdict=row("verdict", np.uint8)[:count], reply=row("reply", np.uint16)[:count],
                    reply_verdict=row("reply_verdict", np.uint8)[:count], allowed=row("allowed", np.uint32), summary=int(r["summary"][0]))

    def _sims(self):
        return int(self.a.engine.status()[2].cpu().numpy()[0])

    def _root(self):
        if not self._rooted:
            self.a.engine.reset(*self.pos)
            self._rooted = True
            return False
        return True

    def search(self, playouts):
        expanded = self._root()
        before = self._sims()
        self.a.engine.search(self.a.forward, int(playouts), root_done=expanded)
        return self._sims() - before

    def lines(self, allowed, n_lines, max_len):
        self._root()
        mask = np.ascontiguousarray(allowed, np.uint32).reshape(1, -1)
        return self.a.read_lines(mask, n_lines, max_len)[0]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.ucci", description="UCCI engine on stdin / stdout.")
    ap.add_argument("--model", default=None, help="checkpoint (own .pt, reference TF bundle, .npz); none = fresh weights")
    ap.add_argument("--blocks", type=int, default=7, help="residual blocks of the net")
    ap.add_argument("--playout", type=int, default=400, help="default of the Playouts option: playouts of a bare `go`")
    ap.add_argument("--search_threads", type=int, default=16, help="simulations in flight per lock-step")
    args = ap.parse_args(argv)
    from .analysis import Analyzer
    from .arena import load_player
    net = load_player(args.model, args.blocks)
    # the node pool is sized once: for the Playouts default or 4096 playouts, whichever is more (a longer search stops expanding
    # when the pool is full and answers from the visits it has)
    analyzer = Analyzer(net, max(args.playout, 4096), 1, width=max(1, min(args.search_threads, 64)))
    UcciEngine(AnalyzerSearcher(analyzer), sys.stdin, sys.stdout, playouts=args.playout).run()


if __name__ == "__main__":
    main()
