"""Host model of self-play under rules="xiangqi" (csrc/cz_selfplay.hip with cz_selfplay_set_rules(1) and
cz_selfplay_set_repetition and cz_selfplay_set_chase) — TEST INFRASTRUCTURE: tests/selfplay_model.py's choice and game end,
with the king-safe filter and the repetition or chase verdict of tests/rootrules_model.py in front of them, at the root only.

  choose_xq_ref      selfplay_model.choose_ref over rootrules_model.safe_children: pi, noise and pick over the king-safe
                     root children alone, gamma[j] belonging to compacted child j
  adjudicate_xq_ref  the ending order (wave_game_end, csrc/cz_internal.h) — repetition verdict, mate, then
                     selfplay_model.adjudicate_ref — and the z values
  replay_line        a forced line on the oracle's boards: the history of keys and check flags and the first verdict
  play_games         whole games of G slots in lock-step (continuous=False) on oracle.Search trees from a given random stream:
                     packed records in ring order, the outcomes, the counters; z of a chase loss is a perpetual check's
"""
import numpy as np

import chase_model as CM
import kingsafe_model as KM
import match_model as MM
import repetition_model as RM
import rootrules_model as RR
import selfplay_model as M

NONE = 0xFFFF


def choose_xq_ref(board, side, labels, visits, temperature, gamma, eps, u):
    """-> (child index among all children, margin, king-safe child indices), or (None, inf, []) when no child is king-safe."""
    idx = RR.safe_children(board, side, labels)
    if not idx:
        return None, float("inf"), idx
    g = None if gamma is None else np.asarray(gamma, np.float64)[:len(idx)]
    j, margin = M.choose_ref(np.asarray(visits, np.int64)[idx], temperature, g, eps, u)
    return idx[j], margin, idx


def adjudicate_xq_ref(verdict, mated, root_side, board, rr, ply, movers, max_plies, stalled=False):
    """The game end of one slot.  verdict / mated: what the choice found on the root it left untouched (root_side to move);
    otherwise board / rr are the position after the move.  -> selfplay_model.Outcome with .how in {"repetition", "perpetual",
    "mate", None}, or None while the game goes on."""
    n = min(int(ply), int(max_plies))
    movers = np.asarray(movers, np.int64)[:n]
    if verdict != RM.NONE:
        if verdict == RM.DRAW:
            o = M.Outcome("draw", n, np.zeros(n))
            o.how = "repetition"
            return o
        winner = M.BLACK if verdict == RM.RED_LOSES else M.RED
        o = M.Outcome("red" if winner == M.RED else "black", n, np.where(movers == winner, 1, -1))
        o.how = "perpetual"
        return o
    if mated:
        winner = 1 - int(root_side)          # the side to move has no king-safe move: it loses
        o = M.Outcome("red" if winner == M.RED else "black", n, np.where(movers == winner, 1, -1))
        o.how = "mate"
        return o
    o = M.adjudicate_ref(board, rr, ply, movers, max_plies, stalled)
    if o is not None:
        o.how = None
    return o


def replay_line(board, side, moves, fold=3, rr=0):
    """Play the labels `moves` from (board, side): -> dict(keys, checks: of positions 0 .. len(moves); ply, code, first: the
    first verdict with window min(rr, ply, 63), or (None, NONE, -1); safe: every move was king-safe; captures)."""
    from oracle import oracle as O
    b, s = np.array(board, np.uint8), int(side)
    history, first_verdict, safe, captures = RR.History(RR.level("xiangqi", fold, False), fold), (None, RM.NONE, -1), True, 0
    for ply in range(len(moves) + 1):
        code, first, _ = history.root(b, s, rr, ply)
        if code != RM.NONE and first_verdict[0] is None:
            first_verdict = (ply, code, first)
        if ply == len(moves):
            break
        mv = int(moves[ply])
        safe = safe and mv in set(int(x) for x in KM.kingsafe(b, s)[0])
        b, cap, _ = O.apply_move(b, mv)
        captures += 1 if cap else 0
        rr = 0 if cap else rr + 1
        s ^= 1
    return dict(keys=history.keys, checks=history.checks, ply=first_verdict[0], code=first_verdict[1], first=first_verdict[2], safe=safe,
                captures=captures)


def _record(board, side, labels, visits, ply):
    from cchess_zero_amd.selfplay import pack_records
    k = len(labels)
    lab = np.full((1, 128), NONE, np.uint16)
    vis = np.zeros((1, 128), np.int64)
    lab[0, :k], vis[0, :k] = labels, visits
    return pack_records(np.asarray(board, np.uint8)[None], np.array([side]), lab, vis, np.array([k]), np.zeros(1), ply=np.array([ply]))[0]


def play_games(fwd, playouts, boards, side, rr, stream, max_plies=512, temperature=1.0, eps=0.25, fold=3, forced=None, cap=1 << 20, chase=False):
    """G games in lock-step, one per slot, parked when they end (SelfPlay(..., continuous=False, rules="xiangqi",
    repetition=fold, chase=chase).step_ply(rand=stream[t], forced=forced[t]) for every t).  fwd: a numpy forward; stream[t] =
    (gamma [G, 128] or None, u [G]) as float32; forced[t] (optional) = labels [G], 0xFFFF = none.  chase=False: the chase records
    are kept, the verdict is the repetition rule's.
    -> dict(records [n, REC_BYTES] in the order the ring receives them, outcomes [(t, slot, Outcome)] in that order (.how may be
    "chase"), stats (the cz_selfplay_stats slots games .. stalled and mates / repetitions / perpetuals / chases), active [G] bool,
    min_margin over the unforced picks, picks (their number), unsafe_plies (plies whose root had a child that is not king-safe),
    keys / checks / records_chase (per slot, the positions' history))."""
    from cchess_zero_amd._lib import REC_BYTES, REC_Z
    from oracle import oracle as O
    G = len(boards)
    finished, active = [], np.ones(G, bool)
    margins, picks, unsafe_plies = [], 0, 0
    level, histories = RR.level("xiangqi", fold, chase), []
    for g in range(G):
        S = O.Search(1, cap)
        S.reset(np.asarray(boards[g], np.uint8)[None], np.array([side[g]], np.uint8), np.array([0 if rr is None else rr[g]], np.int32))
        recs, movers, ply = [], [], 0
        history = RR.History(level, fold, records=True)
        histories.append(history)
        try:
            for t in range(len(stream)):
                MM._search(S, fwd, playouts)
                st = S.root_stats()
                n = int(st["count"][0])
                b, s, r = S.root_state()
                b, s, r = b[0], int(s[0]), int(r[0])
                verdict, mated, stalled, cause = RM.NONE, False, False, CM.CAUSE_NONE
                if n == 0 or int(S.status()[0][0]) & (2 | 4):
                    stalled = True
                else:
                    if level >= RR.REPETITION:
                        verdict, _, cause = history.root(b, s, r, ply)
                    if verdict == RM.NONE:
                        labels, visits = st["label"][0, :n], st["N"][0, :n]
                        gamma = None if stream[t][0] is None else stream[t][0][g]
                        pick, margin, idx = choose_xq_ref(b, s, labels, visits, temperature, gamma, eps, float(stream[t][1][g]))
                        mated = pick is None
                if not (stalled or mated or verdict != RM.NONE):
                    unsafe_plies += 1 if len(idx) < n else 0
                    mv = int(labels[pick])
                    f = NONE if forced is None or forced[t] is None else int(forced[t][g])
                    if f < O.NLABELS:
                        mv = f
                    else:
                        margins.append(margin)
                        picks += 1
                    if ply < max_plies:
                        recs.append(_record(b, s, labels[idx], visits[idx], ply))
                    movers.append(s)
                    ply += 1
                    stalled = mv not in set(int(x) for x in labels)      # BAD_ADVANCE: a forced label that is no root child
                    S.advance(np.array([mv], np.uint16))
                    b, _, r = S.root_state()
                    b, r = b[0], int(r[0])
                o = adjudicate_xq_ref(verdict, mated, s, b, r, ply, movers, max_plies, stalled)
                if o is not None:
                    if cause == CM.CAUSE_CHASE:
                        o.how = "chase"
                    out = np.stack(recs[:o.fin_n]) if o.fin_n else np.zeros((0, REC_BYTES), np.uint8)
                    out[:, REC_Z] = o.z.astype(np.int8).view(np.uint8)
                    finished.append((t, g, o, out))
                    active[g] = False
                    break
        finally:
            S.close()
    finished.sort(key=lambda x: (x[0], x[1]))
    outcomes = [(t, g, o) for t, g, o, _ in finished]
    stats = M.stats_ref([o for _, _, o in outcomes])
    for k, how in (("mates", "mate"), ("repetitions", "repetition"), ("perpetuals", "perpetual"), ("chases", "chase")):
        stats[k] = sum(1 for _, _, o in outcomes if o.how == how)
    records = np.concatenate([r for _, _, _, r in finished]) if finished else np.zeros((0, REC_BYTES), np.uint8)
    return dict(records=records, outcomes=outcomes, stats=stats, active=active, picks=picks, unsafe_plies=unsafe_plies,
                min_margin=min(margins) if margins else float("inf"), keys=[h.keys for h in histories],
                checks=[h.checks for h in histories], records_chase=[h.records for h in histories])
