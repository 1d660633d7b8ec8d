"""State-string <-> board-array conversion, FEN, and WXF / Chinese move notation (host side, tiny).

The reference's state is a FEN-like string: 10 ranks joined by '/', rank 0 first (red / upper-case /
'w' home), digits = runs of empty squares (main.py:585, :705-714, :691-699).  The device format is
uint8[90], sq = y*9 + x, code = 1 + index in 'KARBNPCkarbnpc' (main.py:208), 0 = empty.
"""
import numpy as np

PIECES = ".KARBNPCkarbnpc"
START_STATE = "RNBAKABNR/9/1C5C1/P1P1P1P1P/9/9/p1p1p1p1p/1c5c1/9/rnbakabnr"
_CODE = {c: i for i, c in enumerate(PIECES) if i}
# the reference also accepts 'h'/'H' for knights and 'e'/'E' for bishops in get_legal_moves (main.py:835,857)
_CODE.update({"H": _CODE["N"], "h": _CODE["n"], "E": _CODE["B"], "e": _CODE["b"]})


def state_to_board(state):
    b = np.zeros(90, np.uint8)
    rows = state.split("/")
    if len(rows) != 10:
        raise ValueError("state must have 10 ranks: %r" % state)
    for y, row in enumerate(rows):
        x = 0
        for ch in row:
            if ch.isdigit():
                x += int(ch)
            else:
                if x >= 9 or ch not in _CODE:
                    raise ValueError("bad state string: %r" % state)
                b[y * 9 + x] = _CODE[ch]
                x += 1
        if x != 9:
            raise ValueError("rank %d of %r does not have 9 files" % (y, state))
    return b


def board_to_state(board):
    board = np.asarray(board, np.uint8).reshape(10, 9)
    rows = []
    for y in range(10):
        s, run = "", 0
        for x in range(9):
            c = int(board[y, x])
            if c == 0:
                run += 1
            else:
                if run:
                    s += str(run)
                    run = 0
                s += PIECES[c]
        if run:
            s += str(run)
        rows.append(s)
    return "/".join(rows)


def player_to_side(player):
    return 1 if player == "b" else 0


def side_to_player(side):
    return "b" if side else "w"


# ---- standard Xiangqi FEN ---------------------------------------------------------------------------------------------------
# "<ranks> <side> [- - halfmove fullmove]": rank 9 (black's back rank) first, files a .. i from left to right, upper case red.
# The board array has rank 0 (red's back rank) first and file a at x = 0, so a FEN's rank field is the state string with its
# ranks in reverse order.  Move text is the label string itself (_lib.tables()["labels"]): files a-i, ranks 0-9 with red at
# rank 0 — ICCS coordinates ("h2e2").
START_FEN = "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR w"


def fen_to_position(fen):
    """Standard Xiangqi FEN -> (board uint8[90], side 0 red / 1 black, restrict round).  The side field is w / r (red) or b; the
    optional fields are `- - halfmove fullmove`, the halfmove clock (plies since the last capture) becoming the restrict round.
    E / H are read as B / N.  ValueError on anything else."""
    if not isinstance(fen, str):
        raise ValueError("FEN must be a string: %r" % (fen,))
    f = fen.split()
    if not 1 <= len(f) <= 6:
        raise ValueError("FEN has %d fields: %r" % (len(f), fen))
    ranks = f[0].split("/")
    if len(ranks) != 10:
        raise ValueError("FEN must have 10 ranks: %r" % fen)
    for row in ranks:
        if any(ch.isdigit() and not "1" <= ch <= "9" for ch in row):
            raise ValueError("bad rank %r in FEN %r" % (row, fen))
    board = state_to_board("/".join(reversed(ranks)))
    for king in ("K", "k"):
        if not (board == _CODE[king]).any():
            raise ValueError("FEN without the king %r: %r" % (king, fen))
    side = f[1] if len(f) > 1 else "w"
    if side not in ("w", "r", "b"):
        raise ValueError("side to move must be w, r or b: %r" % fen)
    rr = 0
    if len(f) > 4:
        if not f[4].isdigit():
            raise ValueError("halfmove clock must be a number: %r" % fen)
        rr = int(f[4])
    if len(f) > 5 and not f[5].isdigit():
        raise ValueError("fullmove number must be a number: %r" % fen)
    return board, (1 if side == "b" else 0), rr


def position_to_fen(board, side, rr=0, fullmove=1):
    """(board, side, restrict round) -> "<ranks> <w|b> - - <rr> <fullmove>"."""
    ranks = board_to_state(board).split("/")
    return "%s %s - - %d %d" % ("/".join(reversed(ranks)), "b" if side else "w", int(rr), int(fullmove))


# ---- WXF and Chinese move notation ------------------------------------------------------------------------------------------
# A move in these notations has no coordinates: a piece kind, a file counted from the mover's right (9 - x for red, x + 1 for
# black), a direction and a target file or a distance.  Both are READ to one canonical token, a uint32 of four bytes b0 b1 b2 b3
# (least significant first; include/cchess_hip.h, cz_games_read), with no board: the replay kernel finds the move the token names
# in the position it is played in.  They are WRITTEN here from a board, by the notations' own rules (move_text): that side shares
# nothing with the kernel's matcher and is the independent half of the round trip the tests make.
#   b0  K A E H R C P, or a file digit: the pawn on that file (pawns doubled on two files)
#   b1  the source file digit, or an ordinal on the file: + frontmost, - rearmost, a-e the 1st .. 5th from the front
#   b2  + forward, - backward, = sideways;   b3  a digit: the target file, or the distance of a straight move
_WXF_KIND = {"K": "K", "A": "A", "E": "E", "B": "E", "H": "H", "N": "H", "R": "R", "C": "C", "P": "P"}
_ZH_KIND = {}
for _k, _chars in (("K", "帥帅將将"), ("A", "仕士"), ("E", "相象"), ("H", "傌馬马"), ("R", "俥車车"), ("C", "炮砲包"), ("P", "兵卒")):
    _ZH_KIND.update({c: _k for c in _chars})
_ZH_NUM = "一二三四五六七八九"
_DIGIT = {str(d): str(d) for d in range(1, 10)}
_DIGIT.update({c: str(i + 1) for i, c in enumerate(_ZH_NUM)})
_DIGIT.update({chr(0xFF10 + d): str(d) for d in range(1, 10)})      # full-width
_ZH_DIR = {"進": "+", "进": "+", "退": "-", "平": "="}
_ZH_ORD = {"前": "+", "中": "b", "後": "-", "后": "-"}
_ZH_PIECE = {"K": "帥將", "A": "仕士", "E": "相象", "H": "馬馬", "R": "車車", "C": "炮炮", "P": "兵卒"}   # red, black


def _pack(b0, b1, b2, b3):
    return ord(b0) | ord(b1) << 8 | ord(b2) << 16 | ord(b3) << 24


def token_text(token):
    """The four canonical bytes of a token as text: "C2=5"."""
    return "".join(chr((int(token) >> s) & 0xFF) for s in (0, 8, 16, 24))


def wxf_token(text):
    """A WXF move -> its canonical token.  Read: N for H and B for E, lower case, '.' for '=', the ordinal before the letter
    ("+R=4") as well as after it ("R+=4"), a-e for the 1st .. 5th of a file from the front, and a file digit in the piece's place
    with an ordinal ("3+=4", "+3=4").  ValueError names the text."""
    t = text.strip() if isinstance(text, str) else ""
    bad = ValueError("%r is not a WXF move" % (text,))
    if len(t) != 4:
        raise bad
    a, b, d, n = t
    if a in "+-":                                   # the ordinal in front
        a, b = b, a
    d = "=" if d == "." else d
    if d not in "+-=" or n not in "123456789":
        raise bad
    if a in "123456789":                            # a file in the piece's place: the source is an ordinal
        if not (b in "+-" or b.lower() in "abcde"):
            raise bad
        return _pack(a, b.lower(), d, n)
    kind = _WXF_KIND.get(a.upper())
    if kind is None or not (b in "123456789+-" or b.lower() in "abcde"):
        raise bad
    return _pack(kind, b.lower(), d, n)


def chinese_token(text):
    """A move in Chinese notation -> its canonical token.  Read: both sides' piece characters, traditional and simplified,
    進进 / 退 / 平, Chinese, full-width and ASCII digits, 前 / 中 / 後后 or a numeral in front of the piece ("前炮退二", "二兵平四": the
    second pawn from the front), and a file in the piece's place behind such an ordinal ("前三平四").  ValueError names the text."""
    t = text.strip() if isinstance(text, str) else ""
    bad = ValueError("%r is not a move in Chinese notation" % (text,))
    if len(t) != 4:
        raise bad
    a, b, d, n = t
    d, n = _ZH_DIR.get(d), _DIGIT.get(n)
    if d is None or n is None:
        raise bad
    if a in _ZH_KIND:                               # piece, file
        if b not in _DIGIT:
            raise bad
        return _pack(_ZH_KIND[a], _DIGIT[b], d, n)
    if a in _ZH_ORD:
        o = _ZH_ORD[a]
    elif a in _DIGIT and int(_DIGIT[a]) <= 5:
        o = "abcde"[int(_DIGIT[a]) - 1]
    else:
        raise bad
    if b in _ZH_KIND:                               # ordinal, piece
        return _pack(_ZH_KIND[b], o, d, n)
    if b in _DIGIT:                                 # ordinal, file: the pawn
        return _pack(_DIGIT[b], o, d, n)
    raise bad


NOTATIONS = ("iccs", "wxf", "chinese")
_KIND_OF_CODE = ".KAREHPC"                          # PIECES = ".KARBNPC": B is the elephant, N the horse


def _named(board, side, label):
    """The writer's rule -> (b0, b1, b2, b3, pieces of the kind on the file) or None.  1. the file-digit form if the piece is alone
    of its kind on its file, or is A or E; 2. otherwise the ordinal on the file: + and - for the first and the last, a-e for the
    ones between; 3. for a pawn, when more than one file holds two or more of the mover's pawns, the file in the piece's place.
    None: a side with more than two of a kind that is not the pawn (no notation tells three rooks apart)."""
    from ._lib import tables
    board = np.asarray(board, np.uint8).reshape(90)
    sq = int(tables()["srcdst"][int(label)])
    frm, to = sq & 0xFF, sq >> 8
    fy, fx, ty, tx = frm // 9, frm % 9, to // 9, to % 9
    pc = int(board[frm])
    if not (1 <= pc - 7 * side <= 7):
        raise ValueError("move_text: no piece of the side to move on %s" % tables()["labels"][int(label)][:2])
    kind = _KIND_OF_CODE[pc - 7 * side]
    if kind != "P" and int((board == pc).sum()) > 2:
        return None
    fileno = (lambda x: x + 1) if side else (lambda x: 9 - x)
    dy = (fy - ty) if side else (ty - fy)
    ys = [y for y in range(10) if board[9 * y + fx] == pc]
    ys.sort(reverse=not side)                       # from the front: red's front is the high y
    b0 = kind
    if kind in "AE" or len(ys) == 1:
        b1 = str(fileno(fx))
    else:
        i = ys.index(fy)
        b1 = "+" if i == 0 else "-" if i == len(ys) - 1 else "abcde"[i]
        if kind == "P" and sum(1 for x in range(9) if int((board[x::9] == pc).sum()) >= 2) > 1:
            b0 = str(fileno(fx))
    if dy == 0:
        b2, b3 = "=", fileno(tx)
    else:
        b2, b3 = ("+" if dy > 0 else "-"), (fileno(tx) if kind in "AEH" else abs(dy))
    return b0, b1, b2, str(b3), len(ys)


def move_token(board, side, label):
    """The canonical token the writer's rule gives the move `label` of the position, or None (see move_text)."""
    n = _named(board, side, label)
    return None if n is None else _pack(*n[:4])


def move_text(board, side, label, notation="iccs"):
    """The move `label` of the position (board uint8[90], side 0 red / 1 black) as text: "iccs" the label string ("h2e2"), "wxf"
    ("C2=5") or "chinese" ("炮二平五": traditional characters, Chinese numerals for red and ASCII digits for black).  None only
    if a side has more than two of a kind that is not the pawn: the caller then writes ICCS."""
    from ._lib import tables
    if notation not in NOTATIONS:
        raise ValueError("move_text: notation is one of %r" % (NOTATIONS,))
    if notation == "iccs":
        return tables()["labels"][int(label)]
    n = _named(board, side, label)
    if n is None:
        return None
    b0, b1, b2, b3, on_file = n
    if notation == "wxf":
        return b0 + b1 + b2 + b3
    num = (lambda d: d) if side else (lambda d: _ZH_NUM[int(d) - 1])
    what = num(b0) if b0.isdigit() else _ZH_PIECE[b0][1 if side else 0]
    tail = {"+": "進", "-": "退", "=": "平"}[b2] + num(b3)
    if b1.isdigit():
        return what + num(b1) + tail
    o = "前" if b1 == "+" else "後" if b1 == "-" else "中" if on_file == 3 else _ZH_NUM["abcde".index(b1)]
    return o + what + tail


def line_text(board, side, labels, notation="iccs"):
    """A line of moves from the position (a principal variation) as texts: every move is written in the position it is played
    in, the board stepped on the host from move to move; a move the notation has no text for is written in ICCS."""
    from ._lib import tables
    t = tables()
    if notation not in NOTATIONS:
        raise ValueError("line_text: notation is one of %r" % (NOTATIONS,))
    if notation == "iccs":
        return [t["labels"][int(m)] for m in labels]
    b, s, out = np.array(board, np.uint8).reshape(90), 1 if side else 0, []
    for m in labels:
        out.append(move_text(b, s, int(m), notation) or t["labels"][int(m)])
        sq = int(t["srcdst"][int(m)])
        b[sq >> 8], b[sq & 0xFF] = b[sq & 0xFF], 0
        s ^= 1
    return out
