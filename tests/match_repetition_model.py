"""Host model of an evaluation match under rules="xiangqi" with the repetition rule (csrc/cz_match.hip with
cz_match_set_repetition): tests/match_kingsafe_model.py's game with the history of the game's positions and the verdict of
tests/repetition_model.py in front of the choice."""
import numpy as np

import kingsafe_model as KM
import match_kingsafe_model as XM
import match_model as MM
import repetition_model as RM

MATE, REPETITION, PERPETUAL = 5, 6, 7


def ending(code, a_red):
    """A verdict of the rule -> (reason, result for A)."""
    if code == RM.DRAW:
        return REPETITION, 0
    return PERPETUAL, (-1 if (code == RM.RED_LOSES) == bool(a_red) else 1)


def play_game(players, board, side, rr, game, max_plies, sample_plies=0, seed=0, fold=3, cap=1 << 20, trace=None):
    """match_kingsafe_model.play_game with the repetition rule -> dict(moves, plies, reason, result, a_red).  fold = 0: the
    rule is off, only the history is kept.  trace (a list): receives (ply, first) of the game's verdict."""
    from oracle import oracle as O
    a_red = game % 2 == 0
    trees = [O.Search(1, cap), O.Search(1, cap)]
    for S in trees:
        S.reset(np.asarray(board, np.uint8)[None], np.array([side], np.uint8), np.array([rr], np.int32))
    moves, ply, side = [], 0, int(side)
    keys, checks = [], []
    try:
        while True:
            mover = 0 if (side == 0) == a_red else 1
            S = trees[mover]
            MM._search(S, *players[mover])
            st = S.root_stats()
            n = int(st["count"][0])
            status = int(S.status()[0][0])
            if n == 0 or status & (2 | 4):
                reason, result = MM.adjudicate(None, 0, ply, max_plies, True, a_red)
                break
            b, s, r = S.root_state()
            keys.append(int(O.zhash(b[0], side)))
            checks.append(1 if KM.attacked(b[0], side) else 0)
            if fold:
                code, first = RM.verdict(keys, checks, side, min(int(r[0]), ply, 63), fold)
                if code != RM.NONE:
                    if trace is not None:
                        trace.append((ply, first))
                    reason, result = ending(code, a_red)
                    break
            pick = XM.choose(b[0], side, st["label"][0, :n], st["N"][0, :n], ply, sample_plies, seed, game)
            if pick is None:                    # the mover has children, none king-safe: it loses
                reason, result = MATE, (-1 if mover == 0 else 1)
                break
            mv = int(st["label"][0, pick])
            moves.append(mv)
            ply += 1
            for T in trees:
                T.advance(np.array([mv], np.uint16))
            b, s, r = S.root_state()
            side = int(s[0])
            reason, result = MM.adjudicate(b[0], int(r[0]), ply, max_plies, False, a_red)
            if reason:
                break
    finally:
        for T in trees:
            T.close()
    return dict(moves=moves, plies=ply, reason=reason, result=result, a_red=int(a_red))


def play_match(players, openings, max_plies, sample_plies=0, seed=0, fold=3):
    out = dict(result=[], a_red=[], plies=[], reason=[], moves=[])
    for p in range(len(openings.boards)):
        for c in (0, 1):
            g = play_game(players, openings.boards[p], int(openings.side[p]), int(openings.rr[p]), 2 * p + c, max_plies, sample_plies, seed, fold)
            row = np.full(max_plies, 0xFFFF, np.uint16)
            row[:len(g["moves"])] = g["moves"]
            for k in ("result", "a_red", "plies", "reason"):
                out[k].append(g[k])
            out["moves"].append(row)
    return dict(result=np.array(out["result"], np.int8), a_red=np.array(out["a_red"], np.uint8), plies=np.array(out["plies"], np.int32),
                reason=np.array(out["reason"], np.uint8), moves=np.array(out["moves"], np.uint16).reshape(-1, max_plies))
