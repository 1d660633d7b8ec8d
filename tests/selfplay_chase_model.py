"""Host model of self-play with the perpetual-chase rule (csrc/cz_selfplay.hip with cz_selfplay_set_chase) — TEST
INFRASTRUCTURE: tests/selfplay_rules_model.py's games with the chase record of every root position (tests/chase_model.py)
beside its key and check flag, and chase_model.verdict in front of the choice.  z of a chase loss is a perpetual check's."""
import numpy as np

import chase_model as CM
import kingsafe_model as KM
import match_model as MM
import repetition_model as RM
import selfplay_model as M
import selfplay_rules_model as R

NONE = 0xFFFF


def play_games(fwd, playouts, boards, side, rr, stream, max_plies=512, temperature=1.0, eps=0.25, fold=3, forced=None, cap=1 << 20, chase=True):
    """selfplay_rules_model.play_games with the chase record of every root position and chase_model.verdict (chase=False: the
    records are kept, the verdict is the repetition rule's): SelfPlay(..., continuous=False, rules="xiangqi", repetition=fold,
    chase=chase).step_ply(rand=stream[t], forced=forced[t]) for every t.  An outcome's .how may be "chase"; stats has "chases";
    the result also holds records_chase (per slot, the positions' chase records).  fwd: a numpy forward; stream[t] = (gamma [G, 128]
    or None, u [G]) as float32; forced[t] (optional) = labels [G], 0xFFFF = none.
    -> dict(records [n, REC_BYTES] in the order the ring receives them, outcomes [(t, slot, Outcome)] in that order, stats (the
    cz_selfplay_stats slots games .. stalled and mates / repetitions / perpetuals), active [G] bool, min_margin over the unforced
    picks, picks (their number), unsafe_plies (plies whose root had a child that is not king-safe), keys / checks (per slot, the
    positions' history))."""
    from cchess_zero_amd._lib import REC_BYTES, REC_Z
    from oracle import oracle as O
    G = len(boards)
    finished, active = [], np.ones(G, bool)
    margins, picks, unsafe_plies = [], 0, 0
    all_keys, all_checks, all_recs = [], [], []
    for g in range(G):
        S = O.Search(1, cap)
        S.reset(np.asarray(boards[g], np.uint8)[None], np.array([side[g]], np.uint8), np.array([0 if rr is None else rr[g]], np.int32))
        recs, movers, keys, checks, crecs, ply = [], [], [], [], [], 0
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
                    if fold:
                        keys.append(int(O.zhash(b, s)))
                        checks.append(1 if KM.attacked(b, s) else 0)
                        crecs.append(CM.record(b, s))
                        if chase:
                            verdict, _, cause = CM.verdict(keys, checks, crecs, s, min(r, ply, 63), fold)
                        else:
                            verdict, _ = RM.verdict(keys, checks, s, min(r, ply, 63), fold)
                    if verdict == RM.NONE:
                        labels, visits = st["label"][0, :n], st["N"][0, :n]
                        gamma = None if stream[t][0] is None else stream[t][0][g]
                        pick, margin, idx = R.choose_xq_ref(b, s, labels, visits, temperature, gamma, eps, float(stream[t][1][g]))
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
                        recs.append(R._record(b, s, labels[idx], visits[idx], ply))
                    movers.append(s)
                    ply += 1
                    stalled = mv not in set(int(x) for x in labels)      # BAD_ADVANCE: a forced label that is no root child
                    S.advance(np.array([mv], np.uint16))
                    b, _, r = S.root_state()
                    b, r = b[0], int(r[0])
                o = R.adjudicate_xq_ref(verdict, mated, s, b, r, ply, movers, max_plies, stalled)
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
        all_keys.append(keys)
        all_checks.append(checks)
        all_recs.append(crecs)
    finished.sort(key=lambda x: (x[0], x[1]))
    outcomes = [(t, g, o) for t, g, o, _ in finished]
    stats = M.stats_ref([o for _, _, o in outcomes])
    for k, how in (("mates", "mate"), ("repetitions", "repetition"), ("perpetuals", "perpetual"), ("chases", "chase")):
        stats[k] = sum(1 for _, _, o in outcomes if o.how == how)
    records = np.concatenate([r for _, _, _, r in finished]) if finished else np.zeros((0, REC_BYTES), np.uint8)
    return dict(records=records, outcomes=outcomes, stats=stats, active=active, picks=picks, unsafe_plies=unsafe_plies,
                min_margin=min(margins) if margins else float("inf"), keys=all_keys, checks=all_checks, records_chase=all_recs)
