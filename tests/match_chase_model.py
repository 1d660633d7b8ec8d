"""Host model of an evaluation match with the perpetual-chase rule (csrc/cz_match.hip with cz_match_set_chase) — TEST
INFRASTRUCTURE: tests/match_repetition_model.py's game with the chase record of every position (tests/chase_model.py) beside
its key and check flag, and chase_model.verdict in front of the choice."""
import functools

import numpy as np

import chase_cases as CC
import chase_model as CM
import fakenet
import kingsafe_model as KM
import match_kingsafe_model as XM
import match_model as MM
import match_repetition_model as RMM

MATE, REPETITION, PERPETUAL, CHASE = 5, 6, 7, 9
CHASE_PLAYOUTS = 30


def ending(code, cause, a_red):
    """A verdict of the rule -> (reason, result for A): a chase is scored like a perpetual check, with its own reason."""
    reason, result = RMM.ending(code, a_red)
    return (CHASE if cause == CM.CAUSE_CHASE else reason), result


def play_game(players, board, side, rr, game, max_plies, sample_plies=0, seed=0, fold=3, chase=True, cap=1 << 20, trace=None):
    """match_repetition_model.play_game with the chase record and verdict -> dict(moves, plies, reason, result, a_red, records).
    chase=False: the records are kept, the verdict is the repetition rule's.  trace (a list): receives (ply, first, cause)."""
    from oracle import oracle as O
    a_red = game % 2 == 0
    trees = [O.Search(1, cap), O.Search(1, cap)]
    for S in trees:
        S.reset(np.asarray(board, np.uint8)[None], np.array([side], np.uint8), np.array([rr], np.int32))
    moves, ply, side = [], 0, int(side)
    keys, checks, recs = [], [], []
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
            recs.append(CM.record(b[0], side))
            if fold:
                window = min(int(r[0]), ply, 63)
                if chase:
                    code, first, cause = CM.verdict(keys, checks, recs, side, window, fold)
                else:
                    code, first = RMM.RM.verdict(keys, checks, side, window, fold)
                    cause = CM.CAUSE_NONE
                if code != CM.NONE:
                    if trace is not None:
                        trace.append((ply, first, cause))
                    reason, result = ending(code, cause, a_red)
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
    return dict(moves=moves, plies=ply, reason=reason, result=result, a_red=int(a_red), records=recs)


def play_match(players, boards, side, rr, max_plies, sample_plies=0, seed=0, fold=3, chase=True):
    out = dict(result=[], a_red=[], plies=[], reason=[], moves=[])
    for p in range(len(boards)):
        for c in (0, 1):
            g = play_game(players, boards[p], int(side[p]), int(rr[p]), 2 * p + c, max_plies, sample_plies, seed, fold, chase)
            row = np.full(max_plies, 0xFFFF, np.uint16)
            row[:len(g["moves"])] = g["moves"]
            for k in ("result", "a_red", "plies", "reason"):
                out[k].append(g[k])
            out["moves"].append(row)
    return dict(result=np.array(out["result"], np.int8), a_red=np.array(out["a_red"], np.uint8), plies=np.array(out["plies"], np.int32),
                reason=np.array(out["reason"], np.uint8), moves=np.array(out["moves"], np.uint16).reshape(-1, max_plies))


@functools.lru_cache(maxsize=None)
def fakenet_match(sample_plies, chase=True):
    """The 16-game fakenet match of tests/test_match_repetition_gpu.py (cpu_openings(8, 4, 11), pos/11 at 24 playouts against
    signed/12 at 16, max_plies 160, seed 5, fold 3), replayed on the CPU once per process; read-only."""
    import repetition_cases as RC
    boards, side = RC.cpu_openings(8, 4, 11)
    players = [(fakenet.make_forward("pos", 11), 24), (fakenet.make_forward("signed", 12), 16)]
    out = play_match(players, boards, side, np.zeros(len(boards), np.int32), 160, sample_plies, 5, 3, chase)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- the constructed chase, played by search ------------------------------------------------------------------------------
def steering_forward():
    """A numpy forward on planes [B, 9, 10, 14] that makes a search play chase_cases.CHASE_LINE.  The reference's root never
    counts its own visits, so at the root U = 0 and the choice among the root children is by Q alone: a policy cannot steer it,
    the values do.  Value 0 on the four positions of the line (keyed by fakenet.position_key of their planes), +0.9 for the
    side to move everywhere else: whoever leaves the line hands the other side a good position, so the line's move is every
    root's only child with Q >= 0 and takes the visits left once each child has been tried.  Logits all 1."""
    from oracle import oracle as O
    boards, sides, _ = CC.play_line(CC.CHASE_BOARD, 0, CC.CHASE_LINE[:4])
    keys = np.array([fakenet.position_key(O.encode_planes(boards[i], int(sides[i]))[None])[0] for i in range(4)], np.uint64)

    def forward(planes):
        planes = np.asarray(planes, np.float32)
        if planes.ndim == 3:
            planes = planes[None]
        hit = np.isin(fakenet.position_key(planes), keys)
        return np.ones((planes.shape[0], 2086), np.float32), np.where(hit, np.float32(0.0), np.float32(0.9)).astype(np.float32).reshape(-1, 1)
    return forward


def steering_device_forward():
    import torch
    f = steering_forward()

    def forward(planes):
        lg, v = f(planes.float().cpu().numpy())
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    return forward
