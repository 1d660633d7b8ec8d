"""The model of cz_games_replay (TEST INFRASTRUCTURE): recorded games replayed ply by ply in NumPy over the C oracle's
legal_moves / apply_move (the reference's get_legal_moves and sim_do_action) and tests/kingsafe_model.py, the records packed
by selfplay.pack_records.  It shares no text with cchess_zero_amd/csrc/cz_games.h; the kernel, the host build of its per-game
step and cchess_zero_amd/games.py are held to this file byte for byte."""
import json
import os

import numpy as np

import kingsafe_model as KM
from oracle import oracle as O

OK, ILLEGAL, AFTER_END, BAD_BOARD, BAD_LEN = 0, 1, 2, 3, 4
RED_KING_GONE, BLACK_KING_GONE = 16, 32
REC_BYTES = 608
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def start_board():
    return O.fen_to_board(O.START_FEN)


def refused(board, side):
    """The boards the stand-alone generators answer with count 0xFFFF (include/cchess_hip.h, cz_movegen): more than 16 pieces of
    the side to move, more of a kind than a Xiangqi set holds, or — the oracle raises — a move without a label."""
    own = board[(board >= 8) if side else ((board >= 1) & (board <= 7))].astype(int) - (7 if side else 0)
    cnt = np.bincount(own, minlength=8)   # K 1, A 2, R 3, B 4, N 5, P 6, C 7
    if len(own) > 16 or cnt[1] > 1 or cnt[6] > 5 or (cnt[[2, 3, 4, 5, 7]] > 2).any():
        return True
    try:
        O.legal_moves(board, side)
    except RuntimeError:
        return True
    return False


def legal_list(board, side, rules):
    """-> the position's list at the rule level (None: refused)"""
    if refused(board, side):
        return None
    return KM.kingsafe(board, side)[0] if rules else O.legal_moves(board, side)


def end_flags(board, side):
    f = 0 if refused(board, side) else KM.kingsafe(board, side)[1]
    return f | (0 if (board == 1).any() else RED_KING_GONE) | (0 if (board == 8).any() else BLACK_KING_GONE)


def replay_game(board, side, moves, length, stride, result, rules):
    """One game -> dict(records uint8 [max(length, 0) if length <= stride else 0, 608], valid, status, end_flags, board, side)"""
    from cchess_zero_amd.selfplay import pack_records
    board, side = np.array(board, np.uint8), int(side)
    if length < 0 or length > stride:
        return dict(records=np.zeros((0, REC_BYTES), np.uint8), valid=0, status=BAD_LEN, end_flags=end_flags(board, side), board=board, side=side)
    recs = np.zeros((length, REC_BYTES), np.uint8)
    status, valid = OK, 0
    for i in range(length):
        label = int(moves[i])
        lst = legal_list(board, side, rules)
        if lst is None:
            status = BAD_BOARD
        elif not (board == 1).any() or not (board == 8).any() or (rules and len(lst) == 0):
            status = AFTER_END
        elif label not in [int(x) for x in lst]:
            status = ILLEGAL
        if status != OK:
            break
        labels = np.full((1, 128), 0xFFFF, np.uint16)
        labels[0, :len(lst)] = lst
        visits = np.zeros((1, 128), np.int64)
        visits[0, [int(x) for x in lst].index(label)] = 1
        recs[i] = pack_records(board[None], [side], labels, visits, [len(lst)], [-result if side else result], ply=[i])[0]
        board = O.apply_move(board, label)[0]
        side ^= 1
        valid += 1
    return dict(records=recs, valid=valid, status=status, end_flags=end_flags(board, side), board=board, side=side)


def replay(boards, sides, moves, lens, results, rules, rec_offset=None, total=None, fill=0xA5):
    """The whole call: games [G] -> dict(records [total, 608] (untouched records hold `fill`), valid, status, end_flags,
    final_boards, final_side, per_game: the replay_game dicts).  rec_offset None: the games' records one after the other."""
    G, stride = moves.shape
    if rec_offset is None:
        ln = np.where((lens >= 0) & (lens <= stride), lens, 0)
        rec_offset = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int32) if G else np.zeros(0, np.int32)
        total = int(ln.sum()) if total is None else total
    out = np.full((total, REC_BYTES), fill, np.uint8)
    per = []
    for g in range(G):
        b = start_board() if boards is None else boards[g]
        r = replay_game(b, 0 if sides is None else sides[g], moves[g], int(lens[g]), stride, int(results[g]), rules)
        for i in range(len(r["records"])):
            at = int(rec_offset[g]) + i
            if 0 <= at < total:
                out[at] = r["records"][i]
        per.append(r)
    return dict(records=out, valid=np.array([r["valid"] for r in per], np.int32), status=np.array([r["status"] for r in per], np.uint8),
                end_flags=np.array([r["end_flags"] for r in per], np.uint8), final_boards=np.stack([r["board"] for r in per]),
                final_side=np.array([r["side"] for r in per], np.uint8), per_game=per, rec_offset=rec_offset, total=total)


def golden_games():
    """The reference's own six self-play games (tests/golden/selfplay.npz) as move lists -> (moves uint16 [6, stride], lens,
    results int8 (z is the mover's view: the result is z of a red ply, -z of a black one), the fixture's rows per game)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "selfplay.npz"))
    n = len(json.loads(str(g["meta"])))
    rows = [np.nonzero(g["case"] == c)[0] for c in range(n)]
    stride = max(len(r) for r in rows)
    moves = np.full((n, stride), 0xFFFF, np.uint16)
    results = np.zeros(n, np.int8)
    for c, r in enumerate(rows):
        moves[c, :len(r)] = g["played"][r]
        res = np.where(g["side"][r] == 0, g["z"][r], -g["z"][r])
        assert (res == res[0]).all()
        results[c] = int(res[0])
    return moves, np.array([len(r) for r in rows], np.int32), results, rows, g
