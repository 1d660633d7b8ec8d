"""Analysis of N positions at once: best move, score and principal variations per position.

    python -m cchess_zero_amd.analysis --fen "<fen>" [--fen "<fen>" ...] [--fen-file F] --model M.pt --blocks 7 --playout 400 --lines 3 [--book B.npz]

prints one JSON object per position.  Positions are searched in chunks of `games` trees through one SearchEngine; per chunk:
reset, one Rules.movegen_kingsafe launch for the root masks, `playouts` simulations, one cz_search_lines launch.

What the search is: the reference's king-capture search (a position's value is decided by taking the king, 60 plies without
a capture are a draw), with the Xiangqi rules applied AT THE ROOT — the lines start at king-safe root moves only, and a mover
without a king-safe move is reported as such and not searched.  That is what matches and self-play do under --rules xiangqi
(cz_match_set_rules, cz_selfplay_set_rules); below the root the tree holds pseudo-legal moves.  rules="capture" drops the root
mask.  Scores are Q of the line's first move as the tree holds it, from the mover's view (-1 .. 1).
"""
import argparse
import json

import numpy as np
import torch

from . import _lib
from ._lib import MASK_WORDS, NLABELS, POS_NO_SAFE_MOVE
from .engine import SearchEngine, plane_format, pool_nodes
from .notation import fen_to_position
from .rules import Rules

RULES = ("capture", "xiangqi")


def label_of(move):
    """A move given as its label or its ICCS text -> the label (ValueError for text that is no move of the board)."""
    if isinstance(move, str):
        try:
            return _lib.tables()["label2i"][move]
        except KeyError:
            raise ValueError("no such move: %r" % move)
    return int(move)


def ban_words(ban, G):
    """ban[i] = the moves (labels or text) position i may not start a line with -> uint32 [G, 66], their bits set."""
    words = np.zeros((G, MASK_WORDS), np.uint32)
    for i, moves in enumerate(ban):
        for m in moves or ():
            l = label_of(m)
            if not 0 <= l < NLABELS:
                raise ValueError("no such move label: %r" % (m,))
            words[i, l >> 5] |= np.uint32(1) << np.uint32(l & 31)
    return words


class Analyzer:
    """analyse() for any number of positions, `games` at a time, on one SearchEngine of `games` trees sized for `playouts`."""

    def __init__(self, net, playouts, games, width=1, rules="xiangqi", device=0):
        if rules not in RULES:
            raise ValueError("rules: %s" % " or ".join(RULES))
        if int(games) < 1:
            raise ValueError("an analysis needs at least one tree")
        from .arena import _player   # a PolicyValueNet, the policy_value_network facade or a device forward -> what search() takes
        self.forward, self.playouts = _player((net, playouts))
        self.games, self.rules = int(games), rules
        # the fused net path reads 16-bit planes straight from the select kernel at width 1; k simulations in flight use the
        # reference's float32 planes and the net's full forward
        pd, ch = plane_format(self.forward) if int(width) == 1 else (torch.float32, 14)
        self.engine = SearchEngine(self.games, pool_nodes(self.playouts), device, plane_dtype=pd, channels=ch, width=int(width))
        self.engine.compact = int(width) == 1   # parked positions cost the net nothing
        self.rule_kernels = Rules(ctx=self.engine.ctx)
        self.labels = _lib.tables()["labels"]

    # -- one chunk, stage by stage (analyse() drives them; the UCCI engine steps them) ----------------------------------------
    def root_masks(self, boards, side, ban=None):
        """-> (allowed [G, 66] int32 device tensor or None, flags uint8 [G] host array) of G positions: under rules "xiangqi" the
        king-safe sets (one cz_movegen_kingsafe launch) and the CZ_POS_* flags, under "capture" no mask and no flags; the bits
        of ban[i] cleared."""
        G = len(side)
        allowed, flags = None, np.zeros(G, np.uint8)
        if self.rules == "xiangqi":
            _, _, allowed, pos_flags = self.rule_kernels.movegen_kingsafe(boards, side, want_moves=False)
            flags = pos_flags.cpu().numpy()
        if ban is not None and any(ban):
            if allowed is None:
                allowed = torch.full((G, MASK_WORDS), -1, dtype=torch.int32, device=self.engine.dev)
            allowed = allowed & ~self.engine.ctx.tensor(ban_words(ban, G), torch.int32)
        return allowed, flags

    def read_lines(self, allowed, n_lines, max_len):
        """One cz_search_lines launch -> per tree the list of its lines, dict(pv=[labels], visits=[...], q=[float32 ...])."""
        ln = self.engine.lines_host(n_lines, max_len, allowed)
        out = []
        for g in range(self.engine.G):
            rows = []
            for j in range(n_lines):
                n = int(ln["len"][g, j])
                if n:
                    rows.append(dict(pv=[int(x) for x in ln["moves"][g, j, :n]], visits=[int(x) for x in ln["visits"][g, j, :n]],
                                     q=[np.float32(x) for x in ln["q"][g, j, :n]]))
            out.append(rows)
        return out

    def repetition(self, positions, history, fold=3, chase=False, notation="iccs"):
        """What the repetition rule says about the moves of positions whose games are known: history[i] = the positions of
        game i BEFORE positions[i], the first one first (tuples as analyse() takes them), or None -> per position None, or
        dict(fold, chase, banned=[dict(move, verdict, cause, reply)], forced, wins=[dict(move, cause)]): `banned` the moves that
        lose by the rule (Rules.repetition_moves: verdict "loss" = the move itself completes the fold-th occurrence with the
        mover as the side that checked / chased perpetually, "reply" = the opponent's `reply` does), `forced` = every move
        loses, `wins` the moves after which the opponent has lost.  One batch of hash / in_check / threats over all the games'
        positions, then one cz_repetition_moves launch."""
        from .notation import line_text
        tup = lambda p: fen_to_position(p) if isinstance(p, str) else p
        games = [(i, [tup(q) for q in h] + [tup(p)]) for i, (p, h) in enumerate(zip(positions, history)) if h is not None]
        out = [None] * len(positions)
        if not games:
            return out
        rk = self.rule_kernels
        boards = np.stack([np.asarray(q[0], np.uint8).reshape(90) for _, g in games for q in g])
        side = np.array([1 if q[1] else 0 for _, g in games for q in g], np.uint8)
        keys, checks = rk.hash(boards, side).cpu().numpy(), (rk.in_check(boards, side) & _lib.POS_IN_CHECK).cpu().numpy()
        recs = rk.threats(boards, side).cpu().numpy() if chase else None
        G, stride = len(games), max(len(g) for _, g in games)
        K, C, R = np.zeros((G, stride), np.int64), np.zeros((G, stride), np.uint8), np.zeros((G, stride, 4), np.int64)
        length, window, at = np.zeros(G, np.int32), np.zeros(G, np.int32), 0
        for k, (_, g) in enumerate(games):
            n = len(g)
            K[k, :n], C[k, :n], length[k] = keys[at:at + n], checks[at:at + n], n
            if chase:
                R[k, :n] = recs[at:at + n]
            window[k] = int(g[-1][2]) if len(g[-1]) > 2 else n - 1     # the restrict round: plies since the last capture
            at += n
        last = np.cumsum(length) - 1
        r = rk.repetition_moves(boards[last], side[last], K, C, R if chase else None, length, window, int(fold))
        r = {k: v.cpu().numpy() for k, v in r.items()}
        cause = {_lib.CAUSE_CHECK: "check", _lib.CAUSE_CHASE: "chase"}
        for k, (i, g) in enumerate(games):
            b, sd = boards[last[k]], int(side[last[k]])
            text = lambda l: line_text(b, sd, [int(l) & 0xFFFF], notation)[0]
            loss_m, loss_o = (_lib.REP_BLACK_LOSES, _lib.REP_RED_LOSES) if sd else (_lib.REP_RED_LOSES, _lib.REP_BLACK_LOSES)
            banned, wins = [], []
            for j in range(int(r["count"][k])):
                v, rv, mv = int(r["verdict"][k, j]), int(r["reply_verdict"][k, j]), int(r["moves"][k, j]) & 0xFFFF
                if v & 15 == loss_m:
                    banned.append(dict(move=text(mv), verdict="loss", cause=cause[v >> 4], reply=None))
                elif v & 15 == _lib.REP_NONE and rv:
                    nb = np.array(b, np.uint8, copy=True)
                    src, dst = int(_lib.tables()["srcdst"][mv]) & 0xFF, int(_lib.tables()["srcdst"][mv]) >> 8
                    nb[dst], nb[src] = nb[src], 0
                    banned.append(dict(move=text(mv), verdict="reply", cause=cause[rv >> 4],
                                       reply=line_text(nb, 1 - sd, [int(r["reply"][k, j]) & 0xFFFF], notation)[0]))
                elif v & 15 == loss_o:
                    wins.append(dict(move=text(mv), cause=cause[v >> 4]))
            out[i] = dict(fold=int(fold), chase=bool(chase), banned=banned, forced=bool(int(r["summary"][k]) & _lib.REPMOVES_FORCED), wins=wins)
        return out

    def analyse(self, positions, n_lines=1, max_len=16, ban=None, notation="iccs", mate_plies=0, tablebase=None, book=None, history=None,
                repetition=3, chase=False):
        """positions: FEN strings or (board uint8[90], side, restrict round) tuples, any number; ban: None or, per position, the
        moves no line may start with.  -> per position dict(bestmove, score, lines=[dict(pv=[move text ...], visits, q)], sims,
        flags): lines in rank order (more visits first), visits / q those of the line's first move, bestmove = lines[0].pv[0],
        score = its q; flags = the position's CZ_POS_* bits.  A mover without a king-safe move reports bestmove None with
        POS_NO_SAFE_MOVE in flags and is not searched; so does, without the flag, a position whose every candidate is banned.
        notation: "iccs" (the default: what UCCI tools read), "wxf" or "chinese" — every move of a line written in the position it
        is played in (notation.line_text).
        mate_plies = N > 0 (odd, 1 .. 15): before the search, Rules.mate looks for a continuous-check mate within N plies
        ("checks" mode), and every position's dict gains mate = dict(plies=d, pv=[move text ...]) or mate = None; the search
        and everything it reports are unchanged.
        tablebase = a cchess_zero_amd.tablebase.Tablebase (default None: nothing changes): every position's dict gains tablebase =
        dict(wdl, plies, pv=[move text ...]) — the exact value from the mover's view and the table's principal line — or
        tablebase = None for a position no loaded table covers; the search and everything it reports are unchanged.
        book = a cchess_zero_amd.book.Book (default None: nothing changes): every position's dict gains book = Book.probe's list of
        the position (empty when the book does not hold it); the search and everything it reports are unchanged.
        history = per position the earlier positions of its game or None (default None: nothing changes): every position's dict
        gains repetition = Analyzer.repetition's answer under the fold `repetition` (and the chase rule with `chase`) — the moves
        the repetition rule bans, with their verdicts — or None; the search and everything it reports are unchanged."""
        from .notation import line_text
        pos = [fen_to_position(p) if isinstance(p, str) else p for p in positions]
        if ban is not None and len(ban) != len(pos):
            raise ValueError("ban has one entry per position")
        mates = None
        if mate_plies:
            from .mate import solve
            mates = [dict(plies=m["plies"], pv=m["pv"]) if m["status"] == "mate" else None
                     for m in solve(self.rule_kernels, pos, int(mate_plies), notation=notation)]
        out = []
        for at in range(0, len(pos), self.games):
            chunk = pos[at:at + self.games]
            boards = np.stack([np.asarray(p[0], np.uint8).reshape(90) for p in chunk])
            side = np.array([1 if p[1] else 0 for p in chunk], np.uint8)
            rr = np.array([int(p[2]) if len(p) > 2 else 0 for p in chunk], np.int32)
            eng = self.engine
            eng.reset(boards, side, rr)
            allowed, flags = self.root_masks(boards, side, None if ban is None else ban[at:at + self.games])
            live = (flags & POS_NO_SAFE_MOVE) == 0
            if live.any():
                eng.search(self.forward, self.playouts, active=None if live.all() else eng.ctx.tensor(live.astype(np.uint8), torch.uint8))
            lines = self.read_lines(allowed, n_lines, max_len)
            sims = eng.status()[2].cpu().numpy()
            for g in range(len(chunk)):
                rows = [dict(pv=line_text(boards[g], side[g], r["pv"], notation), visits=r["visits"][0], q=float(r["q"][0]))
                        for r in lines[g]] if live[g] else []
                out.append(dict(bestmove=rows[0]["pv"][0] if rows else None, score=rows[0]["q"] if rows else None, lines=rows,
                                sims=int(sims[g]), flags=int(flags[g])))
        if mates is not None:
            for r, m in zip(out, mates):
                r["mate"] = m
        if tablebase is not None:
            for r, p in zip(out, pos):
                d = tablebase.describe(p[0], 1 if p[1] else 0, notation)
                r["tablebase"] = None if d is None else dict(wdl=d["wdl"], plies=d["plies"], pv=d["pv"])
        if book is not None and pos:
            rows = book.probe(np.stack([np.asarray(p[0], np.uint8).reshape(90) for p in pos]), np.array([1 if p[1] else 0 for p in pos], np.uint8))
            for r, b in zip(out, rows):
                r["book"] = b
        if history is not None:
            if len(history) != len(pos):
                raise ValueError("history has one entry per position")
            for r, h in zip(out, self.repetition(pos, history, repetition, chase, notation)):
                r["repetition"] = h
        return out

    def play(self, position, moves):
        """position (a tuple as analyse() takes it) and ICCS moves -> every position of the line, the first one first; ValueError
        on a move that is not king-safe where it is played."""
        t = _lib.tables()
        out = [(np.asarray(position[0], np.uint8).reshape(90), 1 if position[1] else 0, int(position[2]) if len(position) > 2 else 0)]
        for m in moves:
            b, sd, rr = out[-1]
            l = label_of(m)
            allowed, _ = self.root_masks(b[None], np.array([sd], np.uint8))
            if allowed is not None and not (int(allowed[0, l >> 5]) >> (l & 31)) & 1:
                raise ValueError("illegal move %s" % m)
            src, dst = int(t["srcdst"][l]) & 0xFF, int(t["srcdst"][l]) >> 8
            nb = b.copy()
            capture = nb[dst] != 0
            nb[dst], nb[src] = nb[src], 0
            out.append((nb, 1 - sd, 0 if capture else rr + 1))
        return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.analysis",
                                 description="Best move, score and principal variations of Xiangqi positions; one JSON object per position.")
    ap.add_argument("--fen", action="append", default=[], help="a position as standard Xiangqi FEN (may be given more than once)")
    ap.add_argument("--fen-file", default=None, help="a file with one FEN per line")
    ap.add_argument("--model", default=None, help="checkpoint (own .pt, reference TF bundle, .npz); none = fresh weights")
    ap.add_argument("--blocks", type=int, default=7, help="residual blocks of the net")
    ap.add_argument("--playout", type=int, default=400, help="playouts per position")
    ap.add_argument("--lines", type=int, default=1, help="principal variations per position")
    ap.add_argument("--notation", choices=("iccs", "wxf", "chinese"), default="iccs", help="how the moves of the output are written (default: ICCS)")
    ap.add_argument("--tablebase", metavar="DIR", default=None, help="a directory of endgame tables (python -m cchess_zero_amd.tablebase --build): "
                    "every position also reports its exact value and line from them")
    ap.add_argument("--book", metavar="B.npz", default=None, help="an opening book (python -m cchess_zero_amd.book --build): every position also reports "
                    "its book moves")
    ap.add_argument("--moves", metavar="\"<iccs ...>\"", default=None, help="moves played from every --fen: the position after them is analysed, and "
                    "its output gains \"repetition\": the moves the repetition rule bans in it, given that game")
    ap.add_argument("--repetition", type=int, default=3, help="with --moves: the fold of the repetition rule (2..8, default 3)")
    ap.add_argument("--chase", action="store_true", help="with --moves: the perpetual-chase rule too")
    args = ap.parse_args(argv)
    if args.moves is not None and not 2 <= args.repetition <= 8:
        ap.error("--repetition is 2..8, not %d" % args.repetition)
    fens = list(args.fen)
    if args.fen_file:
        fens += [l.strip() for l in open(args.fen_file) if l.strip()]
    if not fens:
        ap.error("no position: give --fen or --fen-file")
    try:
        pos = [fen_to_position(f) for f in fens]
    except ValueError as e:
        ap.error(str(e))
    from .arena import load_player
    net = load_player(args.model, args.blocks)
    an = Analyzer(net, args.playout, min(len(pos), 8192))
    tb = None
    if args.tablebase:
        from .tablebase import Tablebase
        tb = Tablebase(an.rule_kernels)
        tb.load(args.tablebase)
    bk = None
    if args.book:
        from .book import Book
        bk = Book(an.engine.ctx).load(args.book)
    history = None
    if args.moves is not None:
        try:
            games = [an.play(p, args.moves.split()) for p in pos]
        except ValueError as e:
            ap.error(str(e))
        pos, history = [g[-1] for g in games], [g[:-1] for g in games]
    res = an.analyse(pos, args.lines, notation=args.notation, tablebase=tb, book=bk, history=history, repetition=args.repetition, chase=args.chase)
    for f, r in zip(fens, res):
        print(json.dumps(dict(fen=f, **r), ensure_ascii=args.notation != "chinese"), flush=True)
    return res


if __name__ == "__main__":
    main()
