"""A model of the table set (include/cchess_hip.h: TABLE SETS) and of tablebase adjudication, on tests/tablebase_model.py and
its recorded tables (tests/golden/tablebase_model.npz):

  material_key   the key Tablebase.signatures_of defines, board by board;
  probe          the mixed probe: the value and the place of ONE board against a set of tables given in some order;
  verdict        how a game ends at an adjudicate, (how, loser), from everything wave_game_end is told — the table's value among
                 the other endings, in their precedence.

Nothing here shares code with the library or with cchess_zero_amd.tablebase."""
import numpy as np

import tablebase_model as TM

ILLEGAL, MISS = TM.ILLEGAL, TM.MISS
MAX_SLOTS = 10
# CZ_MATCH_*: why a game ended
KING, RR60, PLY_CAP, ABORTED, MATE, REPETITION, PERPETUAL, CHASE, RESIGN, TABLEBASE = 1, 2, 3, 4, 5, 6, 7, 9, 10, 11
REP_NONE, REP_DRAW, REP_RED_LOSES, REP_BLACK_LOSES = 0, 1, 2, 3


def material_key(board):
    """sum over the piece codes c = 1 .. 14 of min(count of c, 7) << 3 c, and bit 45 when any byte is no piece code"""
    board = np.asarray(board, np.uint8).reshape(90)
    key = (1 << 45) if bool((board > 14).any()) else 0
    for c in range(1, 15):
        key += min(int((board == c).sum()), 7) << (3 * c)
    return key


def signature_key(sig):
    """the key of every board of a signature"""
    return sum(1 << (3 * code) for code, _ in TM.parse(sig))


def probe(tables, order, board, side):
    """-> (value, which): tables {signature: int16 values}, order: the signatures of the set in the order given.  The table's
    value, ILLEGAL for a piece outside its domain, or MISS (which -1) when no signature of the set has the board's pieces."""
    board = np.asarray(board, np.uint8).reshape(90)
    if bool((board > 14).any()) or int((board != 0).sum()) > MAX_SLOTS:
        return MISS, -1
    sig = TM.signature_of(board)
    if sig is None or sig not in order:
        return MISS, -1
    at = TM.rank(sig, board, side)
    return (ILLEGAL if at is None else int(tables[sig][at])), list(order).index(sig)


def covered(value):
    return value != MISS and value != ILLEGAL


def verdict(value, side_to_move, rep=REP_NONE, by_chase=False, mated=False, resigned=False, aborted=False, red_king=True, black_king=True,
            rr=0, ply=0, max_plies=1 << 30):
    """(how, loser) of a game at an adjudicate; loser: the side code that lost, -1 for a draw, an aborted game and a game that
    goes on (how 0).  value: what the table set says of the position after the move, from side_to_move's view (MISS: no set, or
    the slot did not move).  Behind the repetition verdict, the mated mover, the resignation and the aborted game — found at the
    root that was not left —, in front of the king test, the 60-ply rule and the ply cap."""
    if rep == REP_DRAW:
        return REPETITION, -1
    if rep != REP_NONE:
        return (CHASE if by_chase else PERPETUAL), (0 if rep == REP_RED_LOSES else 1)
    if mated:
        return MATE, side_to_move
    if resigned:
        return RESIGN, side_to_move
    if aborted:
        return ABORTED, -1
    if covered(value):
        return TABLEBASE, (1 - side_to_move if value > 0 else side_to_move if value < 0 else -1)
    if not red_king:
        return KING, 0
    if not black_king:
        return KING, 1
    if rr >= 60:
        return RR60, -1
    if ply >= max_plies:
        return PLY_CAP, -1
    return 0, -1


def result_for_a(loser, a_red):
    """A match game's result from A's view: -1 when the losing side is A's colour, +1 when it is B's, 0 for a draw"""
    if loser < 0:
        return 0
    return -1 if (loser == 0) == bool(a_red) else 1
