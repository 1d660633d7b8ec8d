"""State-string <-> board-array conversion (host side, tiny).

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
