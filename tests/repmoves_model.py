"""The model of the two-ply repetition verdicts on root moves (TEST INFRASTRUCTURE): include/cchess_hip.h cz_repetition_moves in
plain Python, on tests/kingsafe_model.py, tests/chase_model.py, tests/repetition_model.py and the C oracle.  cz_repmoves.h and
cz_repetition_moves are held to this file bit for bit.

A game's record is keys / checks (/ records) of positions 0 .. n0, the last one the current position (board, side).  Candidate
j is the j-th king-safe move; it makes position n0 + 1 with window 0 after a capture, else min(w + 1, n0 + 1).  A king-safe
reply makes position n0 + 2, its window by the same step.  Each is judged by the live rule on the record extended by it."""
import numpy as np

import chase_model as CM
import kingsafe_model as KM
import repetition_model as RM
from oracle import oracle as O

NONE, DRAW, RED_LOSES, BLACK_LOSES = RM.NONE, RM.DRAW, RM.RED_LOSES, RM.BLACK_LOSES
REMOVED, FORCED, OPP_LOSES = 1, 2, 4     # CZ_REPMOVES_*
NO_REPLY = 0xFFFF


def judge(keys, checks, recs, side_now, window, fold):
    """The live rule -> code | cause << 4: cz_repetition_chase with records, cz_repetition (a loss: cause check) without."""
    if recs is not None:
        code, _, cause = CM.verdict(keys, checks, recs, side_now, window, fold)
    else:
        code, _ = RM.verdict(keys, checks, side_now, window, fold)
        cause = CM.CAUSE_CHECK if code in (RED_LOSES, BLACK_LOSES) else CM.CAUSE_NONE
    return code | (cause << 4)


class Position:
    """The position after `label` on (board, side): its key at once, its check flag and chase record when they are asked for
    (the rule looks at them only when the key has occurred before)."""

    def __init__(self, board, side, label):
        self.board, self.cap, _ = O.apply_move(board, int(label))
        self.side = 1 - side
        self.key = int(O.zhash(self.board, self.side))
        self._check = self._record = None

    def check(self):
        if self._check is None:
            self._check = 1 if KM.attacked(self.board, self.side) else 0
        return self._check

    def record(self):
        if self._record is None:
            self._record = CM.record(self.board, self.side)
        return self._record


def judge_extended(keys, checks, recs, new, window, fold):
    """The live rule on the record extended by the positions `new` (the last one current, with `window`)"""
    allkeys = keys + [p.key for p in new]
    n = len(allkeys) - 1
    w = max(0, min(window, n))
    if allkeys[n] not in allkeys[n - w:n]:
        return NONE               # no earlier occurrence: no verdict whatever the flags and records are
    return judge(allkeys, checks + [p.check() for p in new], None if recs is None else recs + [p.record() for p in new], new[-1].side, w, fold)


def repetition_moves(board, side, keys, checks, recs=None, window=None, fold=3, wcap=1 << 30):
    """-> dict(moves: the king-safe labels; verdict, reply, reply_verdict: one entry per move; allowed: the labels left;
    summary).  recs None: no chase rule.  wcap: no window grows past it (63 for a slot's ring)."""
    keys, checks = [int(k) for k in keys], [int(c) for c in checks]
    recs = None if recs is None else [[int(x) for x in r] for r in recs]
    n0 = len(keys) - 1
    w = n0 if window is None else max(0, min(int(window), n0))
    loss_m, loss_o = (BLACK_LOSES, RED_LOSES) if side else (RED_LOSES, BLACK_LOSES)
    moves = [int(m) for m in KM.kingsafe(board, side)[0]]
    verdict, reply, reply_verdict, losing = [], [], [], []
    for m in moves:
        c = Position(board, side, m)
        w1 = 0 if c.cap else min(w + 1, n0 + 1, wcap)
        own = judge_extended(keys, checks, recs, [c], w1, fold)
        rp, rv = NO_REPLY, 0
        for r in KM.kingsafe(c.board, c.side)[0]:
            g = Position(c.board, c.side, r)
            w2 = 0 if g.cap else min(w1 + 1, n0 + 2, wcap)
            v = judge_extended(keys, checks, recs, [c, g], w2, fold)
            if v & 15 == loss_m:
                rp, rv = int(r), v
                break
        verdict.append(own); reply.append(rp); reply_verdict.append(rv)
        losing.append(own & 15 == loss_m or (own & 15 == NONE and rv != 0))
    forced = len(moves) > 0 and all(losing)
    removed = any(losing) and not forced
    allowed = [m for m, l in zip(moves, losing) if not (removed and l)]
    summary = (REMOVED if removed else 0) | (FORCED if forced else 0) | (OPP_LOSES if any(v & 15 == loss_o for v in verdict) else 0)
    return dict(moves=moves, verdict=verdict, reply=reply, reply_verdict=reply_verdict, allowed=allowed, summary=summary, losing=losing)


def history_of(boards, sides, chase=True):
    """-> (keys, checks, records or None) as lists, of a line's positions"""
    keys = [int(O.zhash(b, int(s))) for b, s in zip(boards, sides)]
    checks = [1 if KM.attacked(b, int(s)) else 0 for b, s in zip(boards, sides)]
    return keys, checks, ([CM.record(b, int(s)) for b, s in zip(boards, sides)] if chase else None)


def windows_of(boards):
    """The window of every position of a line that starts with window 0: plies since the last capture (the piece count fell)"""
    out, w = [], 0
    for i, b in enumerate(boards):
        w = 0 if i == 0 or np.count_nonzero(b) != np.count_nonzero(boards[i - 1]) else w + 1
        out.append(w)
    return out


def rows(res):
    """A model answer as the arrays of cz_repetition_moves: (moves u16 [128], count, verdict u8 [128], reply u16 [128],
    reply_verdict u8 [128], allowed u32 [66], summary)"""
    n = len(res["moves"])
    moves = np.full(128, 0xFFFF, np.uint16); moves[:n] = res["moves"]
    verdict = np.zeros(128, np.uint8); verdict[:n] = res["verdict"]
    reply = np.full(128, 0xFFFF, np.uint16); reply[:n] = res["reply"]
    rv = np.zeros(128, np.uint8); rv[:n] = res["reply_verdict"]
    return moves, n, verdict, reply, rv, KM.mask_of(res["allowed"]), res["summary"]


# ---- seeded random king-safe walks of few-piece boards: the shared corpus of the CPU and the GPU tests ------------------------
# (FEN of a few-piece board, side to move): found by a search over random boards for walks that reach every kind of verdict
WALK_SETUPS = (("5K3/8c/9/9/9/9/7rR/9/3k5/9", 1), ("9/4K4/9/2r6/9/8P/3p1R3/3k5/2R6/5n3", 0), ("9/9/3K1C3/9/7n1/4N4/9/4k4/7P1/7n1", 1),
               ("9/3K5/9/9/8C/9/9/9/5k2R/1p7", 1), ("9/2R6/4K4/7n1/9/9/9/9/3k5/9", 1), ("9/9/5K3/8p/9/9/9/1n7/1R7/3k5", 0),
               ("9/9/4K4/9/N2r3R1/9/9/3k5/r8/9", 1), ("9/3Kr4/9/9/9/9/9/5kC2/9/8P", 0))
WALK_GAMES, WALK_PLIES, WALK_SEED, WALK_FOLD = 32, 14, 82, 2


def random_walks(games=WALK_GAMES, plies=WALK_PLIES, seed=WALK_SEED):
    """-> a list of (boards [n + 1, 90], sides [n + 1], labels [n]): uniform random king-safe moves, biased towards going back
    (with probability 3/4 a side undoes its last move when that is king-safe), so that positions repeat; a walk stops at a
    mover without a king-safe move."""
    rng = np.random.default_rng(seed)
    sd = O.label_srcdst()
    lut = O.lut()
    out = []
    for g in range(games):
        fen, s = WALK_SETUPS[g % len(WALK_SETUPS)]
        b = O.fen_to_board(fen)
        boards, sides, labels = [b.copy()], [s], []
        for _ in range(plies):
            mv = KM.kingsafe(b, s)[0]
            if len(mv) == 0:
                break
            pick = int(mv[rng.integers(len(mv))])
            if len(labels) >= 2 and rng.integers(4):
                back = int(lut[int(sd[labels[-2]]) >> 8, int(sd[labels[-2]]) & 0xFF])
                if back in mv.tolist():
                    pick = back
            b = O.apply_move(b, pick)[0]
            s ^= 1
            boards.append(b.copy()); sides.append(s); labels.append(pick)
        out.append((np.stack(boards), np.array(sides, np.uint8), labels))
    return out


def walk_counts(cases):
    """How often the model finds each kind of verdict in walk_reference()'s cases -> (dict, games with some verdict, games)"""
    c = dict(draw=0, check=0, chase=0, opponent=0, reply=0, forced=0)
    some, games = set(), set()
    for k in cases:
        r = k["res"]
        loss_m, loss_o = (BLACK_LOSES, RED_LOSES) if k["side"] else (RED_LOSES, BLACK_LOSES)
        games.add(k["game"])
        for v, rv in zip(r["verdict"], r["reply_verdict"]):
            if v & 15 or rv:
                some.add(k["game"])
            c["draw"] += v & 15 == DRAW
            c["check"] += v & 15 == loss_m and v >> 4 == CM.CAUSE_CHECK
            c["chase"] += v & 15 == loss_m and v >> 4 == CM.CAUSE_CHASE
            c["opponent"] += v & 15 == loss_o
            c["reply"] += rv != 0
        c["forced"] += r["summary"] & FORCED != 0
    return c, len(some), len(games)


_CACHE = {}


def walk_reference(fold=WALK_FOLD, seed=WALK_SEED):
    """The model on every prefix of every walk, with the chase rule, computed once per process (read-only): a list of
    dict(board, side, keys, checks, recs, window, fold, res, game, ply, played) — played: the label played next, or None."""
    if (fold, seed) not in _CACHE:
        cases = []
        for g, (boards, sides, labels) in enumerate(random_walks(seed=seed)):
            keys, checks, recs = history_of(boards, sides)
            win = windows_of(boards)
            for i in range(len(boards)):
                res = repetition_moves(boards[i], int(sides[i]), keys[:i + 1], checks[:i + 1], recs[:i + 1], win[i], fold)
                cases.append(dict(board=boards[i], side=int(sides[i]), keys=keys[:i + 1], checks=checks[:i + 1], recs=recs[:i + 1], window=win[i],
                                  fold=fold, res=res, game=g, ply=i, played=labels[i] if i < len(labels) else None))
        _CACHE[fold, seed] = cases
    return _CACHE[fold, seed]


# ---- constructed cases, shared by the CPU and the GPU tests --------------------------------------------------------------------
def case(name, board, side, keys, checks, recs, window, fold):
    return dict(name=name, board=np.asarray(board, np.uint8), side=int(side), keys=[int(k) for k in keys], checks=[int(c) for c in checks],
                recs=None if recs is None else [[int(x) for x in r] for r in recs], window=window, fold=fold)


def line_cases(name, start, side, line, folds, chase, first=0):
    """Every prefix of a line (from position `first` on) as a case, per fold, with and without the chase records"""
    import chase_cases as CC
    boards, sides, _ = CC.play_line(start, side, line)
    boards, sides = boards[first:], sides[first:]
    keys, checks, recs = history_of(boards, sides)
    win = windows_of(boards)
    return [case("%s fold %d %s position %d" % (name, f, "chase" if ch else "check", i), boards[i], sides[i], keys[:i + 1], checks[:i + 1],
                 recs[:i + 1] if ch else None, win[i], f)
            for f in folds for ch in chase for i in range(len(boards))]


def forced_case():
    """Red K d0 is in check from the rook a0 and cannot step aside (d1 is the pawn d2's, e0 stays on the rank); the one king-safe
    move is the bishop e2 to c0, and it uncovers the rook e1's check on k e9.  The record is made up: the position after it has
    been there four plies ago, black was in check after each of red's moves and red not after each of black's: red checks
    perpetually and its only move loses, fold 2."""
    import chase_cases as CC
    b = CC.board(["Be2", "Re1", "ra0", "pd2"], kings=("Kd0", "ke9"))
    moves = KM.kingsafe(b, 0)[0]
    assert len(moves) == 1
    return case("forced", b, 0, [Position(b, 0, moves[0]).key, 7001, 7002, int(O.zhash(b, 0))], [1, 0, 1, 1], None, None, 2)


def made_up_cases():
    """A capture, a cut window and a quiet shuffle on one board: red R a4 can take the pawn a6 or step aside to b4; the record
    holds both positions after, black to move, two plies back (fold 2)."""
    import chase_cases as CC
    b = CC.board(["Ra4", "pa6"])
    lut = O.lut()
    take, quiet = int(lut[CC.sq("a4"), CC.sq("a6")]), int(lut[CC.sq("a4"), CC.sq("b4")])
    k0 = int(O.zhash(b, 0))
    out = []
    for name, m in (("capture", take), ("quiet", quiet)):
        keys = [Position(b, 0, m).key, 4242, Position(b, 0, m).key, k0]
        out.append(case(name, b, 0, keys, [0, 0, 0, 0], None, None, 2))
        out.append(case(name + " window 0", b, 0, keys, [0, 0, 0, 0], None, 0, 2))
        out.append(case(name + " window 2", b, 0, keys, [0, 0, 0, 0], None, 2, 2))
    return out, take, quiet


def wide_case():
    """A position with more than 64 king-safe moves (conftest.open_boards' climbers, as tests/wide_cases.py takes them) and a
    checking move of index >= 64; the record is made up as forced_case's, for that move alone: it loses, fold 2."""
    from conftest import open_boards
    ob, os_ = open_boards(96, 41)
    for i in range(2, 96, 3):
        b, s = ob[i], int(os_[i])
        moves = KM.kingsafe(b, s)[0]
        for j in range(64, len(moves)):
            p = Position(b, s, moves[j])
            if p.check() and not p.cap and (b == 1).any() and (b == 8).any():
                return case("wide", b, s, [p.key, int(O.zhash(b, s))], [1, 0], None, None, 2), j
    raise AssertionError("no wide position with a checking move behind index 63")


def constructed_cases():
    import chase_cases as CC
    import repetition_cases as RC
    out = line_cases("perpetual", RC.perpetual_board(), 0, RC.PERPETUAL_LINE * 3, (2, 3, 4), (False, True))
    out += line_cases("chase", CC.CHASE_BOARD, 0, CC.CHASE_LINE + ["a5a6"], (2, 3), (True,))
    out += line_cases("chase, the chaser completes", CC.CHASE_BOARD, 0, CC.CHASE_LINE + ["a5a6"], (3,), (True, False), first=1)
    out += made_up_cases()[0] + [forced_case(), wide_case()[0]]
    return out


def model_of(c):
    """The model's answer to a case, kept in it"""
    if "res" not in c:
        c["res"] = repetition_moves(c["board"], c["side"], c["keys"], c["checks"], c["recs"], c["window"], c["fold"])
    return c["res"]
