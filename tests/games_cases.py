"""The fault corpus of cz_games_replay (TEST INFRASTRUCTURE): 130 games of stride 48 built on the CPU from oracle playouts —
two full waves of 64 games and a ragged third, the smallest batch with a ragged last group — with every way a recorded game
can go wrong injected, and the model's answer to them (tests/games_model.py) at both rule levels.  corpus() ASSERTS that every
status, every end_flags bit and both rule levels occur: a green test cannot rest on an empty case."""
import functools

import numpy as np

import games_model as GM
import kingsafe_model as KM
from oracle import oracle as O

G, STRIDE = 130, 48
PINNED_FEN = "4K4/4R4/9/9/9/4r4/9/9/9/3k5"      # red to move: the rook on e1 is pinned on the e-file by the rook on e5
TAKES_FEN = "4K4/4r4/9/9/9/9/9/9/9/3k5"         # black to move takes the red king with the rook on e1
MATED_FEN = "3K5/9/9/9/9/9/9/9/1R7/R3k4"        # black to move and mated: rooks on a9 and b8 against the bare king on e9


def _king_takes(board, side, moves):
    dst = (O.label_srcdst()[moves] >> 8).astype(int)
    return [int(m) for m, d in zip(moves, dst) if board[d] in (1, 8)]


@functools.lru_cache(maxsize=None)
def corpus(seed=20240607):
    """-> dict(boards [G, 90], side [G], moves uint16 [G, STRIDE], lens int32 [G], results int8 [G], notes {game: what was
    injected}, model {rules: games_model.replay(...)})"""
    rng = np.random.default_rng(seed)
    l2i = {s: i for i, s in enumerate(O.labels())}
    boards = np.tile(GM.start_board(), (G, 1))
    side = np.zeros(G, np.uint8)
    lens = (np.arange(G) % (STRIDE + 1)).astype(np.int32)      # 0 .. 48, len 0 (game 0) and len = stride (game 48) in wave 0
    results = rng.integers(-1, 2, G).astype(np.int8)
    moves = np.full((G, STRIDE), 0xFFFF, np.uint16)
    notes = {}
    side[5::7] = 1                                              # black moves first from the opening position
    refused = GM.start_board()
    refused[4 * 9 + 0] = 6                                      # a 17th red piece (and a sixth pawn)
    for g, why in ((60, "refused start, a move given"), (98, "refused start, no move given")):
        boards[g], notes[g] = refused, why
    lens[98] = 0
    boards[61], side[61], lens[61], notes[61] = O.fen_to_board(PINNED_FEN), 0, 3, "custom FEN: a pinned rook leaves its file"
    boards[62], side[62], lens[62], notes[62] = O.fen_to_board(MATED_FEN), 1, 2, "custom FEN: a move in a mated position"
    boards[63], side[63], lens[63], notes[63] = O.fen_to_board(MATED_FEN), 0, 0, "the same board, red to move: it can take the king; no move given"
    boards[64], side[64], lens[64], notes[64] = O.fen_to_board(MATED_FEN), 0, 2, "red takes the black king, then a move is given"
    boards[65], side[65], lens[65], notes[65] = O.fen_to_board(TAKES_FEN), 1, 1, "black takes the red king"
    for g in range(G):
        b, s = boards[g].copy(), int(side[g])
        if g in (60, 98):
            moves[g, :lens[g]] = l2i["a0a1"]
            continue
        for i in range(int(lens[g])):
            if g == 61 and i == 0:
                m = l2i["e1d1"]
            elif g == 62 and i == 0:
                m = l2i["e9e8"]
            elif g == 64 and i == 0:
                m = l2i["a9e9"]
            elif g == 65 and i == 0:
                m = l2i["e1e0"]
            else:
                pseudo = O.legal_moves(b, s)
                safe = KM.kingsafe(b, s)[0] if g % 2 else pseudo      # odd games are Xiangqi games for as long as they can be
                takes = _king_takes(b, s, pseudo)
                if g % 2 == 0 and takes and rng.random() < 0.7:
                    m = takes[0]                                       # a capture-rules game ends when a king can be taken
                elif len(safe):
                    m = int(safe[rng.integers(len(safe))])
                elif len(pseudo):
                    m = int(pseudo[rng.integers(len(pseudo))])        # mated, or a king is gone: the moves go on all the same
                else:
                    m = 0
            moves[g, i] = m
            b, s = O.apply_move(b, m)[0], s ^ 1
    # the injected faults, in games of the second and third wave (the first keeps its lengths 0 .. 48 as they are)
    def not_listed(g, i):
        b, s = boards[g].copy(), int(side[g])
        for k in range(i):
            b, s = O.apply_move(b, int(moves[g, k]))[0], s ^ 1
        listed = set(int(x) for x in O.legal_moves(b, s))
        return next(l for l in range(2086) if l not in listed)
    moves[79, 5], notes[79] = not_listed(79, 5), "ply 5: a label that is not in the list"
    moves[71, 0], notes[71] = not_listed(71, 0), "ply 0: a label that is not in the list"
    moves[77, 7], notes[77] = 2086, "ply 7: label 2086"
    moves[73, 3], notes[73] = 0xFFFF, "ply 3: label 0xFFFF"
    moves[129, 10], notes[129] = 0xFFFE, "ply 10 of the last game of the ragged wave: label 0xFFFE"
    lens[74], notes[74] = -1, "len = -1"
    lens[75], notes[75] = STRIDE + 1, "len = stride + 1"
    lens[128], notes[128] = 1 << 30, "len = 2^30 in the ragged wave"
    model = {r: GM.replay(boards, side, moves, lens, results, r) for r in (0, 1)}
    # ---- nothing below may rest on an empty case
    assert set(np.unique(lens[(lens >= 0) & (lens <= STRIDE)])) == set(range(STRIDE + 1)) and lens[0] == 0 and lens[48] == STRIDE
    for r in (0, 1):
        assert set(model[r]["status"].tolist()) == {GM.OK, GM.ILLEGAL, GM.AFTER_END, GM.BAD_BOARD, GM.BAD_LEN}, (r, np.unique(model[r]["status"]))
        for bit in (1, 2, 4, GM.RED_KING_GONE, GM.BLACK_KING_GONE):
            assert (model[r]["end_flags"] & bit).any() or (r == 0 and bit == 4 and (model[1]["end_flags"] & 4).any()), (r, bit)
        assert model[r]["status"][60] == GM.BAD_BOARD and model[r]["status"][98] == GM.OK and model[r]["end_flags"][98] == 0
        assert model[r]["status"][71] == GM.ILLEGAL and model[r]["valid"][71] == 0
        for g, i in ((79, 5), (77, 7), (73, 3), (129, 10)):   # the injected label stops the game (odd games: king-safe playouts, no king falls before)
            assert model[r]["valid"][g] == i and model[r]["status"][g] == GM.ILLEGAL, (r, g, model[r]["valid"][g], model[r]["status"][g])
        assert (model[r]["status"][[74, 75, 128]] == GM.BAD_LEN).all()
    s0, s1, v0, v1 = model[0]["status"], model[1]["status"], model[0]["valid"], model[1]["valid"]
    assert s0[61] == GM.OK and s1[61] == GM.ILLEGAL and v1[61] == 0            # pseudo-legal, not king-safe
    assert s1[62] == GM.AFTER_END and v1[62] == 0 and model[1]["end_flags"][62] & 4 and v0[62] >= 1   # a move in a mated position
    for r in (0, 1):
        assert model[r]["end_flags"][63] & 2 and model[r]["status"][64] == GM.AFTER_END and model[r]["valid"][64] == 1
        assert model[r]["end_flags"][64] & GM.BLACK_KING_GONE and model[r]["status"][65] == GM.OK and model[r]["end_flags"][65] & GM.RED_KING_GONE
    assert ((s1 == GM.ILLEGAL) & (v1 < v0)).sum() >= 5                       # and capture-rules playouts that Xiangqi stops earlier
    assert ((s0 == GM.AFTER_END) & (model[0]["end_flags"] & (GM.RED_KING_GONE | GM.BLACK_KING_GONE) != 0)).sum() >= 3   # a move after a king capture
    assert ((s1 == GM.OK) & (lens > 10)).sum() >= 20 and (side == 1).sum() >= 10
    return dict(boards=boards, side=side, moves=moves, lens=lens, results=results, notes=notes, model=model)
