"""Batched rules ops K1-K3 over device tensors (host side of cz_movegen / cz_apply_move / cz_encode_planes)."""
import os

import numpy as np
import torch

from ._lib import (BF16, F16, F32, MASK_WORDS, MATE_NONE, MAXMOVES, NLABELS, NSQ, POS_CAN_TAKE_KING, POS_IN_CHECK, POS_NO_SAFE_MOVE,
                   CchessHipError, call, out_pointers, tables)
from .engine import Context


RULES = {"capture": 0, "xiangqi": 1}   # cz_match_set_rules / cz_selfplay_set_rules


def check_rule_options(who, rules, repetition, chase, tablebase=None, resign_min_ply=0, resign_playon=None, avoid=False):
    """The options of arena.Match and selfplay.SelfPlay on how a game ends (`who` names the caller in the text): rules before a
    repetition fold, a fold before the chase rule, rules before a table set (anything but None), and the resignation ranges
    (resign_playon: SelfPlay's alone).  Raises ValueError."""
    if rules not in RULES:
        raise ValueError("%s: rules is 'capture' or 'xiangqi', not %r" % (who, rules))
    if isinstance(repetition, bool) or not isinstance(repetition, (int, np.integer)) or not (repetition == 0 or 2 <= repetition <= 8):
        raise ValueError("%s: repetition is 0 (off) or 2..8, not %r" % (who, repetition))
    if repetition and rules != "xiangqi":
        raise ValueError("%s: repetition needs rules='xiangqi' (the check flags come from the king-safe moves)" % who)
    if chase and not repetition:
        raise ValueError("%s: chase needs a repetition fold (a chase is judged on a repeated position)" % who)
    if avoid and not repetition:
        raise ValueError("%s: avoid_repetition needs a repetition fold (a move is judged by the repetition rule)" % who)
    if tablebase is not None and rules != "xiangqi":
        raise ValueError("%s: tablebase needs rules='xiangqi' (a table holds values under xiangqi rules)" % who)
    if int(resign_min_ply) < 0 or not (resign_playon is None or 0.0 <= float(resign_playon) <= 1.0):
        raise ValueError("%s: resign_min_ply >= 0%s" % (who, "" if resign_playon is None else " and 0 <= resign_playon <= 1"))


def tablebase_set(tablebase):
    """A tablebase option (a tablebase.Tablebase, a tablebase.DeviceSet or None) -> (the DeviceSet to attach, the one made here
    from a Tablebase's loaded tables — the caller's to close — or None)."""
    dset = tablebase.device_set() if hasattr(tablebase, "device_set") else tablebase
    return dset, (dset if dset is not tablebase else None)


def add_rule_flags(parser, games):
    """--rules, --repetition, --chase and --tablebase DIR on an argparse parser; games: whose games they rule, for the help"""
    parser.add_argument("--rules", choices=sorted(RULES), default="capture",
                        help="%s: capture = the reference's games (a king is taken); xiangqi = king-safe moves only, a side without one "
                             "is mated" % games)
    parser.add_argument("--repetition", type=int, default=0,
                        help="with --rules xiangqi: a game ends when its position occurs for the N-th time (3 is the usual value): a draw, "
                             "or a loss for the side that checked perpetually; 0 = no repetition rule")
    parser.add_argument("--chase", action="store_true",
                        help="with --repetition: a side that alone chased one unprotected piece with every move of the cycle loses")
    parser.add_argument("--avoid_repetition", action="store_true",
                        help="with --repetition: the mover does not choose a move that loses by that rule (and by --chase) — it completes "
                             "the N-th occurrence with the mover as the perpetual checker / chaser, or a reply to it does — unless every move "
                             "does; one more launch per ply, over all slots (1.65 ms per ply on 8 192 slots, where a ply searches for seconds)")
    parser.add_argument("--tablebase", metavar="DIR", default=None,
                        help="with --rules xiangqi: a game that reaches a position of a table in DIR (python -m cchess_zero_amd.tablebase "
                             "--build) ends there with the table's result")


def check_rule_flags(parser, args, who):
    """The cross-checks of add_rule_flags' arguments: parser.error on a failure -> load(), which reads the tables of --tablebase
    DIR onto the current device (None without the flag; ValueError for a directory without a table) — called once the
    caller's device stands, by every rank itself."""
    try:
        check_rule_options(who, args.rules, args.repetition, args.chase, args.tablebase, avoid=getattr(args, "avoid_repetition", False))
    except ValueError as e:
        parser.error(str(e))
    if args.tablebase and not os.path.isdir(args.tablebase):
        parser.error("--tablebase: %s is no directory" % args.tablebase)

    def load():
        if not args.tablebase:
            return None
        from .tablebase import Tablebase
        tb = Tablebase()
        if not tb.load(args.tablebase):
            raise ValueError("--tablebase: no table in %s" % args.tablebase)
        return tb
    return load


def set_rule_options(prefix, handle, rules, repetition, chase, avoid=False):
    """<prefix>_set_rules / _set_repetition / _set_chase / _set_avoid on a match or a self-play context, in the order the library
    asks for; an option that is off is left alone."""
    for name, value in (("rules", RULES[rules]), ("repetition", int(repetition)), ("chase", int(bool(chase))), ("avoid", int(bool(avoid)))):
        if value:
            call("%s_set_%s" % (prefix, name), handle, value)


def root_rules_history(prefix, handle, ctx, G):
    """(keys u64 [G, 64], checks u8 [G, 64]) on the host: the slots' position rings of a match or a self-play context
    (<prefix>_history; repetition != 0), position i of a slot's game at [i & 63]."""
    pk, pc = out_pointers(prefix + "_history", handle, 2)
    return ctx.download(pk, np.uint64, (G, 64)), ctx.download(pc, np.uint8, (G, 64))


def root_rules_chase_history(prefix, handle, ctx, G):
    """chase u64 [G, 64, 4] on the host: the slots' rings of chase records (<prefix>_chase_history; chase=True), position i of a
    slot's game at [i & 63] — Rules.threats of that position."""
    return ctx.download(out_pointers(prefix + "_chase_history", handle, 1)[0], np.uint64, (G, 64, 4))


# the start position (main.py:585: RNBAKABNR/9/1C5C1/P1P1P1P1P/9/9/p1p1p1p1p/1c5c1/9/rnbakabnr) as piece codes, sq = 9 y + x
START_BOARD = np.array([3, 5, 4, 2, 1, 2, 4, 5, 3] + [0] * 9 + [0, 7, 0, 0, 0, 0, 0, 7, 0] + [6, 0, 6, 0, 6, 0, 6, 0, 6] + [0] * 18 +
                       [13, 0, 13, 0, 13, 0, 13, 0, 13] + [0, 14, 0, 0, 0, 0, 0, 14, 0] + [0] * 9 + [10, 12, 11, 9, 8, 9, 11, 12, 10], np.uint8)


def random_positions(rules, G, seed, max_ply=80):
    """Seeded uniform-random playouts from the start position, ply ~ U[0, max_ply] per game, all on the GPU (K1 movegen ->
    random pick -> K2 apply); a move that would capture a king is not played (both kings stay on the board).  The synthetic
    positions of SURVEY 8(d) -> (boards [G,90] u8, side [G] u8, restrict_round [G] i32), device tensors."""
    dev = rules.dev
    gen = torch.Generator(device=dev).manual_seed(seed)
    boards = torch.from_numpy(np.tile(START_BOARD, (G, 1))).to(dev)
    side = torch.zeros(G, dtype=torch.uint8, device=dev)
    rr = torch.zeros(G, dtype=torch.int32, device=dev)
    target = torch.randint(0, max_ply + 1, (G,), generator=gen, device=dev)
    alive = torch.ones(G, dtype=torch.bool, device=dev)
    for ply in range(max_ply):
        moves, count, _ = rules.movegen(boards, side, want_mask=False)
        cnt = count.to(torch.int64) & 0xFFFF
        go = alive & (target > ply) & (cnt > 0)
        r = (torch.rand(G, generator=gen, device=dev) * cnt.clamp(min=1)).to(torch.int64).clamp(max=127)
        pick = moves.gather(1, r.unsqueeze(1)).squeeze(1)
        nb, ns = boards.clone(), side.clone()
        lab = torch.where(go, pick, torch.full_like(pick, -1))
        cap, term = rules.apply_move(nb, ns, lab)
        ok = go & (term == 0)
        boards = torch.where(ok.unsqueeze(1), nb, boards)
        side = torch.where(ok, ns, side)
        rr = torch.where(ok, torch.where(cap != 0, torch.zeros_like(rr), rr + 1), rr)
        alive = alive & (ok | ~go)
    return boards.contiguous(), side.contiguous(), rr.contiguous()


class Rules:
    def __init__(self, ctx=None, device=0):
        self.ctx = ctx or Context(1, 2, device)
        self.dev = self.ctx.device

    def _dev(self, a, dtype):
        return self.ctx.tensor(a, dtype)

    def movegen(self, boards, side, want_mask=True, want_moves=True, pad=True, strict=False):
        """GameBoard.get_legal_moves for G positions -> (moves [G,128] i16(u16 bits), count [G], mask [G,66] i32).
        want_moves=False: only the legal-move SET (mask) and the count — the mask-only kernel (k_movegen_mask), moves is None.
        pad=False (CZ_MOVES_NO_PAD): rows are valid up to their count only, the rest of the (uninitialised) buffer is not written.
        strict=True: raise if a board answered count 0xFFFF (not a Xiangqi set: its list / mask row is undefined; include/
        cchess_hip.h) — synchronises; without it a caller checks `count == -1` (0xFFFF as int16) itself before it reads rows."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        G = boards.shape[0]
        moves = torch.empty((G, MAXMOVES), dtype=torch.int16, device=self.dev) if want_moves else None
        count = torch.empty(G, dtype=torch.int16, device=self.dev)
        mask = torch.empty((G, MASK_WORDS), dtype=torch.int32, device=self.dev) if want_mask else None
        if pad:
            self.ctx.call("cz_movegen", boards, side, G, moves, count, mask)
        else:
            self.ctx.call("cz_movegen_ex", boards, side, G, moves, count, mask, 1)
        if strict:
            self.check_counts(count)
        return moves, count, mask

    def movegen_kingsafe(self, boards, side, want_mask=True, want_moves=True, pad=True):
        """The king-safe moves of G positions (cz_movegen_kingsafe: get_legal_moves' list without the moves that leave the
        mover's king attacked) -> (moves [G,128] i16(u16 bits) or None, count [G], mask [G,66] i32 or None, pos_flags [G] u8:
        POS_IN_CHECK | POS_CAN_TAKE_KING | POS_NO_SAFE_MOVE).  pad=False: CZ_MOVES_NO_PAD, as in movegen.  A board movegen
        refuses answers count -1 (0xFFFF) here too."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        G = boards.shape[0]
        moves = torch.empty((G, MAXMOVES), dtype=torch.int16, device=self.dev) if want_moves else None
        count = torch.empty(G, dtype=torch.int16, device=self.dev)
        mask = torch.empty((G, MASK_WORDS), dtype=torch.int32, device=self.dev) if want_mask else None
        pos_flags = torch.empty(G, dtype=torch.uint8, device=self.dev)
        self.ctx.call("cz_movegen_kingsafe", boards, side, G, moves, count, mask, pos_flags, 0 if pad else 1)
        return moves, count, mask, pos_flags

    def checks(self, boards, side, want_moves=True, pad=True):
        """The king-safe moves of G positions that GIVE CHECK (cz_movegen_checks: movegen_kingsafe's list, in its order, without
        the moves after which the other side is not attacked) -> (moves [G,128] i16(u16 bits) or None, count [G] i16, pos_flags
        [G] u8).  pos_flags are the position's own, as movegen_kingsafe returns them: POS_NO_SAFE_MOVE speaks of all king-safe
        moves.  pad=False: CZ_MOVES_NO_PAD.  A board movegen refuses answers count -1 (0xFFFF) and flags 0."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        G = boards.shape[0]
        moves = torch.empty((G, MAXMOVES), dtype=torch.int16, device=self.dev) if want_moves else None
        count = torch.empty(G, dtype=torch.int16, device=self.dev)
        pos_flags = torch.empty(G, dtype=torch.uint8, device=self.dev)
        self.ctx.call("cz_movegen_checks", boards, side, G, moves, count, pos_flags, 0 if pad else 1)
        return moves, count, pos_flags

    def in_check(self, boards, side):
        """-> pos_flags [G] u8 alone (bit 0: the side to move is in check, bit 1: it can take the king, bit 2: it has no
        king-safe move): the launch that builds neither list nor set."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        pos_flags = torch.empty(boards.shape[0], dtype=torch.uint8, device=self.dev)
        self.ctx.call("cz_movegen_kingsafe", boards, side, boards.shape[0], None, None, None, pos_flags, 0)
        return pos_flags

    def repetition(self, keys, in_check, side, length=None, window=None, fold=3):
        """Repetition and perpetual check on G game records (cz_repetition): keys [G, stride] i64 (cz_hash of every position,
        position 0 the opening), in_check [G, stride] u8 (the side to move is attacked: bit 0 of in_check()'s flags), side [G] u8
        (the side to move in the current position), length [G] i32 (positions recorded; None: stride), window [G] i32 (how
        many earlier positions count; None: all) -> (verdict [G] u8: REP_NONE / REP_DRAW / REP_RED_LOSES / REP_BLACK_LOSES,
        first [G] i32: the earlier occurrence the cycle starts from, -1 without a verdict)."""
        keys = self._dev(keys, torch.int64)
        keys = keys.reshape(-1, keys.shape[-1])
        G, stride = keys.shape
        in_check = self._dev(in_check, torch.uint8).reshape(G, stride)
        side = self._dev(side, torch.uint8).reshape(G)
        length = torch.full((G,), stride, dtype=torch.int32, device=self.dev) if length is None else self._dev(length, torch.int32).reshape(G)
        window = None if window is None else self._dev(window, torch.int32).reshape(G)
        verdict = torch.empty(G, dtype=torch.uint8, device=self.dev)
        first = torch.empty(G, dtype=torch.int32, device=self.dev)
        self.ctx.call("cz_repetition", keys, in_check, stride, length, window, side, G, int(fold), verdict, first)
        return verdict, first

    def threats(self, boards, side):
        """The chase record of G positions (cz_threats) -> [G, 4] i64 (u64 bits): words 0, 1 the pieces of the side to move that
        the other side threatens (squares 0 .. 63, 64 .. 89: an unprotected or more valuable piece under a king-safe attack by
        a rook, cannon, knight, advisor or bishop that is no exchange offer), words 2, 3 the squares of the side to move.  A
        board movegen refuses answers four zero words."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        chase = torch.empty((boards.shape[0], 4), dtype=torch.int64, device=self.dev)
        self.ctx.call("cz_threats", boards, side, boards.shape[0], chase)
        return chase

    def repetition_chase(self, keys, in_check, chase, side, length=None, window=None, fold=3):
        """repetition() with the perpetual-chase verdict behind it (cz_repetition_chase): chase [G, stride, 4] i64 is
        threats() of every position -> (verdict [G] u8, first [G] i32, cause [G] u8: CAUSE_NONE / CAUSE_CHECK / CAUSE_CHASE).
        Perpetual check by one side outranks a chase by the other; a side that alone chases one piece with every move of the
        cycle loses."""
        keys = self._dev(keys, torch.int64)
        keys = keys.reshape(-1, keys.shape[-1])
        G, stride = keys.shape
        in_check = self._dev(in_check, torch.uint8).reshape(G, stride)
        chase = self._dev(chase, torch.int64).reshape(G, stride, 4)
        side = self._dev(side, torch.uint8).reshape(G)
        length = torch.full((G,), stride, dtype=torch.int32, device=self.dev) if length is None else self._dev(length, torch.int32).reshape(G)
        window = None if window is None else self._dev(window, torch.int32).reshape(G)
        verdict = torch.empty(G, dtype=torch.uint8, device=self.dev)
        first = torch.empty(G, dtype=torch.int32, device=self.dev)
        cause = torch.empty(G, dtype=torch.uint8, device=self.dev)
        self.ctx.call("cz_repetition_chase", keys, in_check, chase, stride, length, window, side, G, int(fold), verdict, first, cause)
        return verdict, first, cause

    def repetition_moves(self, boards, side, keys, in_check, chase=None, length=None, window=None, fold=3):
        """What repetition_chase() would answer after every king-safe move of G positions and after every king-safe reply to
        it (cz_repetition_moves, one launch): boards [G, 90], side [G] the current positions; keys, in_check, chase, length,
        window, fold the games' records as repetition_chase() takes them, the current position being the record's last one
        (chase None: no chase rule, as repetition()) -> a dict of device tensors: `moves` [G, 128] i16(u16 bits) and `count`
        [G] i16 as movegen_kingsafe; `verdict` [G, 128] u8, REP_* | CAUSE_* << 4 of the position after move j; `reply`
        [G, 128] i16(u16 bits) and `reply_verdict` [G, 128] u8, the first reply whose verdict is a loss for the mover (-1 / 0:
        none); `allowed` [G, 66] i32, the king-safe set without the moves that lose — by their own verdict, or, their own
        being REP_NONE, by a reply — or the whole set when every move loses; `summary` [G] u8 of REPMOVES_REMOVED / _FORCED /
        _OPP_LOSES."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        G = boards.shape[0]
        side = self._dev(side, torch.uint8).reshape(G)
        keys = self._dev(keys, torch.int64).reshape(G, -1)
        stride = keys.shape[1]
        in_check = self._dev(in_check, torch.uint8).reshape(G, stride)
        chase = None if chase is None else self._dev(chase, torch.int64).reshape(G, stride, 4)
        length = torch.full((G,), stride, dtype=torch.int32, device=self.dev) if length is None else self._dev(length, torch.int32).reshape(G)
        window = None if window is None else self._dev(window, torch.int32).reshape(G)
        out = dict(moves=torch.empty((G, MAXMOVES), dtype=torch.int16, device=self.dev), count=torch.empty(G, dtype=torch.int16, device=self.dev),
                   verdict=torch.empty((G, MAXMOVES), dtype=torch.uint8, device=self.dev),
                   reply=torch.empty((G, MAXMOVES), dtype=torch.int16, device=self.dev),
                   reply_verdict=torch.empty((G, MAXMOVES), dtype=torch.uint8, device=self.dev),
                   allowed=torch.empty((G, MASK_WORDS), dtype=torch.int32, device=self.dev), summary=torch.empty(G, dtype=torch.uint8, device=self.dev))
        self.ctx.call("cz_repetition_moves", boards, side, keys, in_check, chase, stride, length, window, G, int(fold), out["moves"], out["count"],
                      out["verdict"], out["reply"], out["reply_verdict"], out["allowed"], out["summary"])
        return out

    @staticmethod
    def check_counts(count):
        """Raises if any position answered count 0xFFFF (k_movegen_list / k_movegen_mask refuse boards that are not a Xiangqi
        set; their rows are undefined and must not be consumed)."""
        bad = (count == -1).nonzero().flatten()
        if bad.numel():
            raise CchessHipError("cz_movegen: %d position(s) are not a Xiangqi set (count 0xFFFF), first at index %d: their move rows are undefined"
                                 % (int(bad.numel()), int(bad[0])))

    def apply_move(self, boards, side, labels, hash_=None):
        """In-place GameBoard.sim_do_action for G games -> (captured [G] u8, terminal [G] i8)."""
        G = boards.shape[0]
        assert boards.is_cuda and side.is_cuda and boards.dtype == torch.uint8 and boards.is_contiguous()
        labels = self._dev(labels, torch.int16)
        cap = torch.empty(G, dtype=torch.uint8, device=self.dev)
        term = torch.empty(G, dtype=torch.int8, device=self.dev)
        self.ctx.call("cz_apply_move", boards, side, labels, G, hash_, cap, term)
        return cap, term

    def _child_offsets(self, count, G):
        """-> (offsets int32 [G + 1]: the exclusive prefix sum of the counts, a refused board's -1 as 0; their total)"""
        offsets = torch.zeros(G + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(self._dev(count, torch.int16).reshape(G).clamp(min=0), 0, out=offsets[1:])
        T = int(offsets[-1].item())
        if T >= 2 ** 31:
            raise ValueError("Rules.successors: %d children do not fit one call (offsets are int32): pass fewer parents" % T)
        return offsets.to(torch.int32), T

    def successors(self, boards, side, moves, count, offsets=None):
        """Every successor of G positions (cz_successors): moves [G,128] i16 and count [G] i16 as movegen / movegen_kingsafe
        return them (padded or not; count -1, a refused board, has no children) -> (boards [T,90] u8, side [T] u8, captured
        [T] u8, parent [T] i32, label [T] i16), T the sum of the counts: child offsets[g] + j is parent g after moves[g][j], in
        list order.  Reading T back is the call's only synchronisation.  offsets: the int32 [G + 1] prefix sum of the counts, for a
        caller that has it already (mate)."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        G = boards.shape[0]
        moves = self._dev(moves, torch.int16).reshape(G, MAXMOVES)
        offsets, T = self._child_offsets(count, G) if offsets is None else (offsets, int(offsets[-1].item()))
        out = torch.empty((T, NSQ), dtype=torch.uint8, device=self.dev)
        cside = torch.empty(T, dtype=torch.uint8, device=self.dev)
        cap = torch.empty(T, dtype=torch.uint8, device=self.dev)
        parent = torch.empty(T, dtype=torch.int32, device=self.dev)
        label = torch.empty(T, dtype=torch.int16, device=self.dev)
        self.ctx.call("cz_successors", boards, side, G, moves, offsets, T, out, cside, cap, parent, label)
        return out, cside, cap, parent, label

    PERFT_CHUNK = 1 << 17

    def perft(self, boards, side, depth, stats=False, chunk=None):
        """Perft under Xiangqi rules (king-safe moves, movegen_kingsafe) of N root positions, all in one pass -> a dict of int64
        numpy arrays [N, depth + 1], column d the tally over the move sequences of length d: `nodes` their number, and with
        stats=True `captures` (sequences whose last move takes a piece), `checks` (positions with POS_IN_CHECK) and `mates`
        (POS_NO_SAFE_MOVE).  Column 0 is the root itself.  A root movegen refuses raises CchessHipError.
        The tree is walked depth first in slices of at most `chunk` parents (default PERFT_CHUNK = 131 072: 2 048 groups, eight
        waves on every CU); a slice's lists and children live until its subtree is done, so the peak is bounded by
        depth x chunk x (256 + 128 x 106) bytes — 128 children of 90 + 16 bytes per parent, 1.8 GB per level at the default,
        never reached: ~40 children per parent make it ~0.6 GB — not by the tree (133 M positions, 12 GB, at depth 5).
        Without stats the last ply is counted, not made: the count-only form of movegen_kingsafe on the frontier of depth - 1."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8).reshape(-1)
        N, depth, chunk = boards.shape[0], int(depth), int(chunk or self.PERFT_CHUNK)
        if depth < 0 or chunk < 1:
            raise ValueError("Rules.perft: depth >= 0 and chunk >= 1")
        names = ("nodes", "captures", "checks", "mates") if stats else ("nodes",)
        tally = {k: torch.zeros((N, depth + 1), dtype=torch.int64, device=self.dev) for k in names}
        tally["nodes"][:, 0] = 1

        def add(name, d, root, w):   # tally[name][root, d] += w, position by position
            if N == 1:
                tally[name][0, d] += w.sum(dtype=torch.int64)
            else:
                tally[name][:, d] += torch.bincount(root, weights=w.to(torch.float64), minlength=N).to(torch.int64)   # exact below 2^53

        def flags_of(d, root, pf):
            add("checks", d, root, pf & POS_IN_CHECK != 0)
            add("mates", d, root, pf & POS_NO_SAFE_MOVE != 0)

        def walk(b, s, root, d):   # the positions of depth d < depth, a root index each
            for lo in range(0, b.shape[0], chunk):
                bb, ss, rr = b[lo:lo + chunk], s[lo:lo + chunk], root[lo:lo + chunk]
                if d == depth - 1 and not stats:
                    _, cnt, _, _ = self.movegen_kingsafe(bb, ss, want_mask=False, want_moves=False)
                    if d == 0:
                        self.check_counts(cnt)
                    add("nodes", d + 1, rr, cnt.clamp(min=0))
                    continue
                mv, cnt, _, pf = self.movegen_kingsafe(bb, ss, want_mask=False, pad=False)
                if d == 0:
                    self.check_counts(cnt)
                if stats:
                    flags_of(d, rr, pf)
                cb, cs, cap, par, _ = self.successors(bb, ss, mv, cnt)
                del mv
                cr = rr[par.to(torch.int64)]
                add("nodes", d + 1, cr, torch.ones_like(cr))
                if stats:
                    add("captures", d + 1, cr, cap != 0)
                del cap, par
                if d + 1 < depth:
                    walk(cb, cs, cr, d + 1)
                elif stats and cb.shape[0]:
                    flags_of(depth, cr, self.in_check(cb, cs))

        root = torch.arange(N, dtype=torch.int64, device=self.dev)
        if depth == 0:
            _, cnt, _, pf = self.movegen_kingsafe(boards, side, want_mask=False, want_moves=False)
            self.check_counts(cnt)
            if stats:
                flags_of(0, root, pf)
        elif N:
            walk(boards, side, root, 0)
        return {k: v.cpu().numpy() for k, v in tally.items()}

    def mate_backup(self, offsets, child_dist, child_label, child_pv=None, mode=0):
        """The AND/OR step of the mate search over child ranges (cz_mate_backup): offsets int32 [G + 1] as successors lays the
        children out, child_dist i16 [T] (plies until the defender is mated, MATE_NONE = not proven), child_label i16 [T],
        child_pv i16 [T, W] or None (W = 0) -> (dist i16 [G], pv i16(u16 bits) [G, W + 1]).  mode 0, the attacker to move: 1 + the
        minimum over the proven children, MATE_NONE without one; mode 1, the defender: 0 without children, MATE_NONE when a
        child is not proven, else 1 + the maximum.  pv: the label of the FIRST child that attains the value, then its line;
        all -1 (0xFFFF) when dist is 0 or MATE_NONE."""
        offsets = self._dev(offsets, torch.int32).reshape(-1)
        G = offsets.shape[0] - 1
        child_dist = self._dev(child_dist, torch.int16).reshape(-1)
        T = child_dist.shape[0]
        child_label = self._dev(child_label, torch.int16).reshape(T)
        W = 0 if child_pv is None else int(child_pv.shape[-1])
        child_pv = self._dev(child_pv, torch.int16).reshape(T, W) if W else None
        dist = torch.empty(G, dtype=torch.int16, device=self.dev)
        pv = torch.empty((G, W + 1), dtype=torch.int16, device=self.dev)
        self.ctx.call("cz_mate_backup", offsets, G, T, child_dist if T else None, child_label if T else None, child_pv if T else None, W, int(mode), dist, pv)
        return dist, pv

    MATE_MAX_PLIES = 15

    def mate(self, boards, side, plies, attacker="checks", chunk=None, node_limit=None):
        """Forced mate within `plies` (odd, 1 .. 15) for the side to move of N root positions -> a dict of numpy arrays:
        `status` u8 (0 no mate within plies, 1 mate, 2 bad root — movegen refuses it, a king is missing or the mover can already
        take the king —, 3 node_limit reached before the root was decided), `dist` i16 (plies until the defender is mated,
        MATE_NONE without a proven mate), `pv` u16 [N, plies] (the line, 0xFFFF behind it) and `nodes` i64 (positions made
        for the root).
        attacker="checks": the attacker plays king-safe moves that give check only (checks()) — the continuous-check mate of
        Xiangqi puzzles; "all": every king-safe move.  The defender always has every king-safe move; a defender without one is
        mated (dist 0, stalemate loses too), one at the horizon is not proven.  The attacker takes the FIRST move in list order
        with the shortest mate, the defender the FIRST with the longest.  Repetition and perpetual-check rules are NOT applied
        inside the proof: a forced mate within `plies` is a mate.
        ONE PASS at `plies`, no iterative deepening: a distance within the horizon is the exact shortest mate whatever the
        horizon (by induction over the plies left: a node's value is its true distance when that fits, MATE_NONE otherwise),
        so deepening over 1, 3, 5, ... would answer the same, line included.
        The tree is walked depth first in slices of at most `chunk` parents like perft (default PERFT_CHUNK); every slice hands
        (dist, pv) of its nodes back through mate_backup, so the tree is never held whole.  At the attacker's last ply the
        children are only asked for their flags: no lists, no grandchildren.  node_limit: once that many positions have been
        made over the call, no further slice is expanded and every root with an unexpanded node below it answers status 3
        (None: no limit); a root decided before that keeps its answer."""
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8).reshape(-1)
        N, plies, chunk = boards.shape[0], int(plies), int(chunk or self.PERFT_CHUNK)
        if plies < 1 or plies > self.MATE_MAX_PLIES or plies % 2 == 0 or chunk < 1:
            raise ValueError("Rules.mate: plies is odd, 1 .. %d, and chunk >= 1" % self.MATE_MAX_PLIES)
        if attacker not in ("checks", "all"):
            raise ValueError("Rules.mate: attacker is 'checks' or 'all', not %r" % (attacker,))
        nodes = torch.zeros(N, dtype=torch.int64, device=self.dev)
        cut = torch.zeros(N, dtype=torch.bool, device=self.dev)
        made = [0]

        def walk(b, s, root, p, attack):   # the nodes of one level, p plies left -> (dist i16 [n], pv i16 [n, p])
            n = b.shape[0]
            dist = torch.full((n,), MATE_NONE, dtype=torch.int16, device=self.dev)
            pv = torch.full((n, p), -1, dtype=torch.int16, device=self.dev)
            for lo in range(0, n, chunk):
                bb, ss, rr = b[lo:lo + chunk], s[lo:lo + chunk], root[lo:lo + chunk]
                if node_limit is not None and made[0] >= node_limit:
                    cut[rr] = True
                    continue
                if attack and attacker == "checks":
                    mv, cnt, _ = self.checks(bb, ss, pad=False)
                else:
                    mv, cnt, _, _ = self.movegen_kingsafe(bb, ss, want_mask=False, pad=False)
                offsets, T = self._child_offsets(cnt, bb.shape[0])
                cb, cs, _, par, label = self.successors(bb, ss, mv, cnt, offsets)
                del mv
                cr = rr[par.to(torch.int64)]
                del par
                made[0] += T
                nodes.index_add_(0, cr, torch.ones_like(cr))
                if p == 1:     # the attacker's last ply: a child is mated or it is not proven
                    mated = self.in_check(cb, cs) & POS_NO_SAFE_MOVE != 0
                    cd, cpv = torch.where(mated, 0, MATE_NONE).to(torch.int16), None
                else:
                    cd, cpv = walk(cb, cs, cr, p - 1, not attack)
                del cb, cs
                dist[lo:lo + chunk], pv[lo:lo + chunk] = self.mate_backup(offsets, cd, label, cpv, 0 if attack else 1)
            return dist, pv

        _, cnt, _, pf = self.movegen_kingsafe(boards, side, want_mask=False, want_moves=False)
        bad = (cnt < 0) | (pf & POS_CAN_TAKE_KING != 0) | ~(boards == 1).any(1) | ~(boards == 8).any(1)
        good = (~bad).nonzero().flatten()
        dist = torch.full((N,), MATE_NONE, dtype=torch.int16, device=self.dev)
        pv = torch.full((N, plies), -1, dtype=torch.int16, device=self.dev)
        if good.numel():
            dist[good], pv[good] = walk(boards[good], side[good], good, plies, True)
        status = torch.where(bad, 2, torch.where(cut, 3, torch.where(dist != MATE_NONE, 1, 0))).to(torch.uint8)
        proven = status == 1
        dist = torch.where(proven, dist, torch.full_like(dist, MATE_NONE))
        pv = torch.where(proven.unsqueeze(1), pv, torch.full_like(pv, -1))
        return dict(status=status.cpu().numpy(), dist=dist.cpu().numpy(), pv=pv.cpu().numpy().view(np.uint16), nodes=nodes.cpu().numpy())

    def divide(self, board, side, depth):
        """Perft of ONE position split by its first move -> {ICCS label: the move sequences of length `depth` that start with
        it}, in list order: perft(depth - 1) over the root's successors, one pass."""
        if int(depth) < 1:
            raise ValueError("Rules.divide: depth >= 1")
        board = self._dev(board, torch.uint8).reshape(1, NSQ)
        side = self._dev(side, torch.uint8).reshape(1)
        mv, cnt, _, _ = self.movegen_kingsafe(board, side, want_mask=False, pad=False)
        self.check_counts(cnt)
        cb, cs, _, _, label = self.successors(board, side, mv, cnt)
        nodes = self.perft(cb, cs, int(depth) - 1)["nodes"][:, -1] if cb.shape[0] else []
        names = tables()["labels"]
        return {names[int(l)]: int(n) for l, n in zip(label.cpu().numpy().view(np.uint16), nodes)}

    def hash(self, boards, side):
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        h = torch.empty(boards.shape[0], dtype=torch.int64, device=self.dev)
        self.ctx.call("cz_hash", boards, side, boards.shape[0], h)
        return h

    def encode_planes(self, boards, side, dtype=torch.float32, channels=14, quirk_q1=True):
        boards = self._dev(boards, torch.uint8).reshape(-1, NSQ)
        side = self._dev(side, torch.uint8)
        G = boards.shape[0]
        out = torch.empty((G, 9, 10, channels), dtype=dtype, device=self.dev)
        self.ctx.call("cz_encode_planes", boards, side, G, out, {torch.bfloat16: BF16, torch.float16: F16}.get(dtype, F32), channels, 1 if quirk_q1 else 0)
        return out
