"""Host model of an evaluation match under rules="xiangqi" (csrc/cz_match.hip with cz_match_set_rules(1)): tests/match_model.py's
search, choice, adjudication and queue, with the king-safe filter of tests/kingsafe_model.py in front of the choice and the
mate ending."""
import numpy as np

import kingsafe_model as KM
import match_model as MM

MATE = 5


def safe_children(board, side, labels):
    """Indices, in generation order, of the root children whose move is king-safe on (board, side)."""
    safe = set(int(x) for x in KM.kingsafe(board, side)[0])
    return [i for i, l in enumerate(labels) if int(l) in safe]


def choose(board, side, labels, visits, ply, sample_plies, seed, game):
    """-> child index among all children (match_model.choose over the king-safe ones), or None: no king-safe child."""
    idx = safe_children(board, side, labels)
    if not idx:
        return None
    return idx[MM.choose(np.asarray(visits)[idx], ply, sample_plies, seed, game)]


def play_game(players, board, side, rr, game, max_plies, sample_plies=0, seed=0, cap=1 << 20):
    """match_model.play_game under xiangqi rules -> dict(moves, plies, reason, result, a_red)."""
    from oracle import oracle as O
    a_red = game % 2 == 0
    trees = [O.Search(1, cap), O.Search(1, cap)]
    for S in trees:
        S.reset(np.asarray(board, np.uint8)[None], np.array([side], np.uint8), np.array([rr], np.int32))
    moves, ply, side = [], 0, int(side)
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
            pick = choose(S.root_state()[0][0], side, st["label"][0, :n], st["N"][0, :n], ply, sample_plies, seed, game)
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


def play_match(players, openings, max_plies, sample_plies=0, seed=0):
    out = dict(result=[], a_red=[], plies=[], reason=[], moves=[])
    for p in range(len(openings.boards)):
        for c in (0, 1):
            g = play_game(players, openings.boards[p], int(openings.side[p]), int(openings.rr[p]), 2 * p + c, max_plies, sample_plies, seed)
            row = np.full(max_plies, 0xFFFF, np.uint16)
            row[:len(g["moves"])] = g["moves"]
            for k in ("result", "a_red", "plies", "reason"):
                out[k].append(g[k])
            out["moves"].append(row)
    return dict(result=np.array(out["result"], np.int8), a_red=np.array(out["a_red"], np.uint8), plies=np.array(out["plies"], np.int32),
                reason=np.array(out["reason"], np.uint8), moves=np.array(out["moves"], np.uint16).reshape(-1, max_plies))
