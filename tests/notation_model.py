"""The model of cz_games_read (TEST INFRASTRUCTURE): the rule by which a WXF / Chinese token names a move of a position, restated
in NumPy from include/cchess_hip.h over the C oracle's move lists and tests/kingsafe_model.py, and the replay of token games
around it on the pattern of tests/games_model.py.  It shares no text with cchess_zero_amd/csrc/cz_notation.h and none with the
writer (cchess_zero_amd/notation.py: move_text): the kernel, the host build of its decode and the writer's round trip are held
to this file."""
import numpy as np

import games_model as GM
from oracle import oracle as O

OK, ILLEGAL, AFTER_END, BAD_BOARD, BAD_LEN, AMBIGUOUS = 0, 1, 2, 3, 4, 5
REC_BYTES = 608
KINDS = "KAREHPC"          # piece codes 1 .. 7 of the red pieces: K A R E(lephant, 'B') H(orse, 'N') P C; black + 7
DIGITS, ORDINALS = "123456789", "+-abcde"
_SRCDST = None


def srcdst():
    global _SRCDST
    if _SRCDST is None:
        _SRCDST = np.asarray(O.label_srcdst(), np.int64)
    return _SRCDST


def token(text):
    """four characters -> the uint32"""
    assert len(text) == 4
    return sum(ord(c) << (8 * i) for i, c in enumerate(text))


class Position:
    """a position and its list: per listed move what a token can ask about it"""

    def __init__(self, board, side, lst):
        self.lst = np.asarray(lst, np.int64)
        sd = srcdst()[self.lst]
        frm, to = sd & 0xFF, sd >> 8
        fy, fx, ty, tx = frm // 9, frm % 9, to // 9, to % 9
        self.side = side
        self.code = np.asarray(board, np.int64)[frm]
        self.ffile = fx + 1 if side else 9 - fx
        self.tfile = tx + 1 if side else 9 - tx
        self.fwd = fy - ty if side else ty - fy
        self.straight = tx == fx
        grid = np.asarray(board, np.int64).reshape(10, 9)
        self.on_file = np.zeros(len(self.lst), np.int64)     # the mover's pieces of the kind on the source's file
        self.rank = np.zeros(len(self.lst), np.int64)        # the source's place among them, 0 = frontmost
        for i in range(len(self.lst)):
            ys = np.nonzero(grid[:, fx[i]] == self.code[i])[0]
            ys = ys if side else ys[::-1]                    # the front is the low y for black, the high y for red
            self.on_file[i] = len(ys)
            self.rank[i] = list(ys).index(fy[i])

    def matching(self, tok):
        """-> the listed labels the token names"""
        c0, c1, c2, c3 = (chr((int(tok) >> s) & 0xFF) for s in (0, 8, 16, 24))
        if len(self.lst) == 0 or c3 not in DIGITS or c2 not in "+-=":
            return []
        if c0 in DIGITS:
            if c1 not in ORDINALS:
                return []
            kind, ok = "P", self.ffile == int(c0)
        elif c0 in KINDS:
            if c1 not in ORDINALS and c1 not in DIGITS:
                return []
            kind, ok = c0, np.ones(len(self.lst), bool)
        else:
            return []
        ok = ok & (self.code == KINDS.index(kind) + 1 + 7 * self.side)
        if c1 in DIGITS:
            ok = ok & (self.ffile == int(c1))
        else:
            want = 0 if c1 == "+" else self.on_file - 1 if c1 == "-" else "abcde".index(c1)
            ok = ok & (self.on_file >= 2) & (self.rank == want)
        d = int(c3)
        if c2 == "=":
            ok = ok & (self.fwd == 0) & (self.tfile == d) & (kind not in "AEH")
        else:
            ok = ok & (self.fwd > 0 if c2 == "+" else self.fwd < 0)
            ok = ok & ((self.tfile == d) if kind in "AEH" else (self.straight & (np.abs(self.fwd) == d)))
        return [int(x) for x in self.lst[ok]]


def replay_game(board, side, tokens, length, stride, result, rules):
    """One game of tokens -> games_model.replay_game's dict, and labels uint16 [stride]: what every made ply decoded to"""
    from cchess_zero_amd.selfplay import pack_records
    board, side = np.array(board, np.uint8), int(side)
    out_labels = np.full(stride, 0xFFFF, np.uint16)
    if length < 0 or length > stride:
        return dict(records=np.zeros((0, REC_BYTES), np.uint8), valid=0, status=BAD_LEN, end_flags=GM.end_flags(board, side), board=board, side=side,
                    labels=out_labels)
    recs = np.zeros((length, REC_BYTES), np.uint8)
    status, valid = OK, 0
    for i in range(length):
        tok = int(tokens[i])
        lst = GM.legal_list(board, side, rules)
        label = None
        if lst is None:
            status = BAD_BOARD
        elif not (board == 1).any() or not (board == 8).any() or (rules and len(lst) == 0):
            status = AFTER_END
        elif tok < 65536:
            label = tok if tok in [int(x) for x in lst] else None
            status = OK if label is not None else ILLEGAL
        else:
            named = Position(board, side, lst).matching(tok)
            status = OK if len(named) == 1 else ILLEGAL if not named else AMBIGUOUS
            label = named[0] if len(named) == 1 else None
        if status != OK:
            break
        labels = np.full((1, 128), 0xFFFF, np.uint16)
        labels[0, :len(lst)] = lst
        visits = np.zeros((1, 128), np.int64)
        visits[0, [int(x) for x in lst].index(label)] = 1
        recs[i] = pack_records(board[None], [side], labels, visits, [len(lst)], [-result if side else result], ply=[i])[0]
        out_labels[i] = label
        board = O.apply_move(board, label)[0]
        side ^= 1
        valid += 1
    return dict(records=recs, valid=valid, status=status, end_flags=GM.end_flags(board, side), board=board, side=side, labels=out_labels)


def replay(boards, sides, tokens, lens, results, rules, rec_offset=None, total=None, fill=0xA5):
    """The whole call, as games_model.replay: and labels_out uint16 [G, stride]"""
    G, stride = tokens.shape
    if rec_offset is None:
        ln = np.where((lens >= 0) & (lens <= stride), lens, 0)
        rec_offset = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int32) if G else np.zeros(0, np.int32)
        total = int(ln.sum()) if total is None else total
    out = np.full((total, REC_BYTES), fill, np.uint8)
    per = []
    for g in range(G):
        b = GM.start_board() if boards is None else boards[g]
        r = replay_game(b, 0 if sides is None else sides[g], tokens[g], int(lens[g]), stride, int(results[g]), rules)
        for i in range(len(r["records"])):
            at = int(rec_offset[g]) + i
            if 0 <= at < total:
                out[at] = r["records"][i]
        per.append(r)
    return dict(records=out, valid=np.array([r["valid"] for r in per], np.int32), status=np.array([r["status"] for r in per], np.uint8),
                end_flags=np.array([r["end_flags"] for r in per], np.uint8), final_boards=np.stack([r["board"] for r in per]),
                final_side=np.array([r["side"] for r in per], np.uint8), labels_out=np.stack([r["labels"] for r in per]), per_game=per,
                rec_offset=rec_offset, total=total)
