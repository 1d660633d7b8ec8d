"""Host model of resignation in the match and in self-play (csrc/cz_match.hip cz_match_set_resign, csrc/cz_selfplay.hip
cz_selfplay_set_resign) — TEST INFRASTRUCTURE, plain Python on the CPU oracle, built on tests/match_model.py,
tests/selfplay_model.py and tests/selfplay_rules_model.py.

  uniform          the play-on draw of a slot's game: match_model.uniform's construction over (seed, slot, game_no)
  root_value       the value a mover resigns on: Q of the most visited candidate child (first maximum of N), or None when that
                   child has no visit
  hist_bin         the histogram bin of a lowest value: 64 bins of width 1/32 over [-1, 1), float32 arithmetic as the kernel's
  suggest_brute    suggest_resign_threshold by brute force over the bin edges
  play_match_game  match_model.play_game with the judgement between the mate exit and the choice
  play_match       match_model.play_match over play_match_game
  play_selfplay    G slots in lock-step from a given random stream, parked or re-seeded, at every rule level, with play-on
                   games, `would`, the four counters and the histogram
"""
import functools

import numpy as np

import chase_model as CM
import fakenet
import match_model as MM
import repetition_model as RM
import rootrules_model as RR
import selfplay_model as M
import selfplay_rules_model as XS

RESIGN = 10                   # CZ_MATCH_RESIGN
NONE = 0xFFFF
STATS = ("resigned", "playon_games", "playon_would_resign", "playon_false_positives")


def uniform(seed, slot, game_no):
    """u in [0, 1) of game `game_no` of slot `slot`: the game plays on when u < playon_fraction."""
    h = MM.splitmix64((int(seed) & MM.M64) ^ MM.splitmix64(((int(slot) << 32) | int(game_no)) & MM.M64))
    return (h >> 11) * 2.0 ** -53


def root_value(visits, q):
    """visits / q of the candidate children in generation order -> float32 Q of the most visited one, None without a visit."""
    visits = np.asarray(visits, np.int64)
    j = int(np.argmax(visits))            # the first maximum, as wave_most_visited
    return np.float32(q[j]) if visits[j] > 0 else None


def hist_bin(q):
    b = int(np.floor((np.float32(q) + np.float32(1.0)) * np.float32(32.0)))
    return min(max(b, 0), 63)


def suggest_brute(hist, target_fp, min_samples=100):
    """The largest edge -1 + b / 32, b in 0..64, with at most target_fp of the entries below it; None below min_samples."""
    hist = [int(x) for x in hist]
    total = sum(hist)
    if total < min_samples or total == 0:
        return None
    best = None
    for b in range(65):
        if sum(hist[:b]) / total <= target_fp:
            best = -1.0 + b / 32.0
    return best


# ---- the match ---------------------------------------------------------------------------------------------------------------
def play_match_game(players, board, side, rr, game, max_plies, threshold, min_ply=0, sample_plies=0, seed=0, rules="capture", fold=0,
                    chase=False, cap=1 << 20):
    """match_model.play_game with resignation: after the repetition verdict and the mate, before the choice, the mover resigns
    when the Q of its most visited candidate is below `threshold` (float32 compare) — reason RESIGN, a loss for the mover, no
    move logged.  -> dict(moves, plies, reason, result, a_red, resigner: the side that resigned or -1)."""
    from oracle import oracle as O
    level = RR.level(rules, fold, chase)
    a_red = game % 2 == 0
    trees = [O.Search(1, cap), O.Search(1, cap)]
    for S in trees:
        S.reset(np.asarray(board, np.uint8)[None], np.array([side], np.uint8), np.array([rr], np.int32))
    moves, ply, side, resigner = [], 0, int(side), -1
    history = RR.History(level, fold)
    thr = None if threshold is None else np.float32(threshold)
    try:
        while True:
            mover = 0 if (side == 0) == a_red else 1
            S = trees[mover]
            MM._search(S, *players[mover])
            st = S.root_stats()
            n = int(st["count"][0])
            if n == 0 or int(S.status()[0][0]) & (2 | 4):
                reason, result = MM.adjudicate(None, 0, ply, max_plies, True, a_red)
                break
            b, s, r = S.root_state()
            if level >= RR.REPETITION:
                code, first, cause = history.root(b[0], side, r[0], ply)
                if code != RM.NONE:
                    reason, result = MM.ending(code, cause, a_red)
                    break
            idx = RR.safe_children(b[0], side, st["label"][0, :n]) if level >= RR.KINGSAFE else list(range(n))
            if not idx:
                reason, result = MM.MATE, (-1 if mover == 0 else 1)
                break
            if thr is not None and ply >= min_ply:
                q = root_value(st["N"][0, :n][idx], st["Q"][0, :n][idx])
                if q is not None and q < thr:
                    reason, result, resigner = RESIGN, (-1 if mover == 0 else 1), side
                    break
            pick = idx[MM.choose(st["N"][0, :n][idx], ply, sample_plies, seed, game)]
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
    return dict(moves=moves, plies=ply, reason=reason, result=result, a_red=int(a_red), resigner=resigner)


def play_match(players, openings, max_plies, threshold, min_ply=0, sample_plies=0, seed=0, rules="capture", fold=0, chase=False):
    """Every game of the openings -> match_model.play_match's arrays, and resigner [n] (the side that resigned, -1: none)."""
    games = [play_match_game(players, openings.boards[p], int(openings.side[p]), int(openings.rr[p]), 2 * p + c, max_plies, threshold, min_ply,
                             sample_plies, seed, rules, fold, chase) for p in range(len(openings.boards)) for c in (0, 1)]
    moves = np.full((len(games), max_plies), NONE, np.uint16)
    for row, g in zip(moves, games):
        row[:len(g["moves"])] = g["moves"]
    col = lambda k, dtype: np.array([g[k] for g in games], dtype)
    return dict(result=col("result", np.int8), a_red=col("a_red", np.uint8), plies=col("plies", np.int32), reason=col("reason", np.uint8),
                moves=moves, resigner=col("resigner", np.int8))


@functools.lru_cache(maxsize=None)
def fakenet_match(threshold, rules="capture", fold=0, chase=False, min_ply=0):
    """The 16-game fixture match of match_model.fakenet_match (same players, openings, max_plies and seed, sample_plies 0) with
    resignation at `threshold`, replayed once per process and setting; read-only."""
    players = [(fakenet.make_forward("pos", 11), 24), (fakenet.make_forward("signed", 12), 16)]
    out = play_match(players, MM.fakenet_openings(), 160, threshold, min_ply, 0, 5, rules, fold, chase)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- self-play ---------------------------------------------------------------------------------------------------------------
class _Slot:
    """The per-slot resignation state of cz_selfplay_set_resign."""

    def __init__(self, g, rs):
        self.g, self.game_no = g, 0
        self.fresh(rs)

    def fresh(self, rs):
        self.playon = uniform(rs["seed"], self.g, self.game_no) < rs["playon"]
        self.minq = [np.float32(2.0), np.float32(2.0)]
        self.would = 0


def play_selfplay(fwd, playouts, boards, side, rr, stream, rules="capture", fold=0, chase=False, continuous=False, max_plies=512,
                  temperature=1.0, eps=0.25, forced=None, resign=None, retune=None, cap=1 << 20, preset=None):
    """G slots in lock-step (SelfPlay(..., continuous=continuous, rules=rules, repetition=fold, chase=chase, resign=...,
    resign_min_ply=..., resign_playon=..., seed=...).step_ply(rand=stream[t], forced=forced[t]) for every t).
    resign: None (off) or dict(threshold, min_ply, playon, seed); retune: {t: threshold} applied before step t
    (SelfPlay.set_resign_threshold).  stream / forced as selfplay_rules_model.play_games.  preset: per slot, hand-set ring keys
    of the slot's first game (rootrules_model.History), or None.
    -> dict(records in ring order, outcomes [(t, slot, Outcome)] (.how "resign" for a resigned game, .playon, .would, .game_no),
    stats (games .. stalled, and mates / repetitions / perpetuals / chases), resign_stats (the four counters), hist int64 [64],
    active [G] bool, min_margin over the unforced picks, game_no [G] at the end)."""
    from cchess_zero_amd._lib import REC_BYTES, REC_Z
    from oracle import oracle as O
    G = len(boards)
    level = RR.level(rules, fold, chase)
    finished, active, margins = [], np.ones(G, bool), []
    counters, hist, game_nos = dict.fromkeys(STATS, 0), np.zeros(64, np.int64), np.zeros(G, np.int64)
    for g in range(G):
        S = O.Search(1, cap)
        start = (np.asarray(boards[g], np.uint8)[None], np.array([side[g]], np.uint8), np.array([0 if rr is None else rr[g]], np.int32))
        S.reset(*start)
        recs, movers, ply = [], [], 0
        history = RR.History(level, fold, preset=None if preset is None else preset[g])
        rs = None if resign is None else dict(resign)
        slot = None if rs is None else _Slot(g, rs)
        try:
            for t in range(len(stream)):
                if rs is not None and retune and t in retune:
                    rs["threshold"] = retune[t]
                MM._search(S, fwd, playouts)
                st = S.root_stats()
                n = int(st["count"][0])
                b, s, r = S.root_state()
                b, s, r = b[0], int(s[0]), int(r[0])
                verdict, mated, stalled, resigned, cause = RM.NONE, False, False, False, CM.CAUSE_NONE
                f = NONE if forced is None or forced[t] is None else int(forced[t][g])
                if n == 0 or int(S.status()[0][0]) & (2 | 4):
                    stalled = True
                else:
                    if level >= RR.REPETITION:
                        verdict, _, cause = history.root(b, s, r, ply)
                    if verdict == RM.NONE:
                        labels, visits = st["label"][0, :n], st["N"][0, :n]
                        idx = RR.safe_children(b, s, labels) if level >= RR.KINGSAFE else list(range(n))
                        mated = not idx
                    if verdict == RM.NONE and not mated and rs is not None and rs["threshold"] is not None and f >= O.NLABELS \
                            and ply >= rs["min_ply"]:
                        q = root_value(visits[idx], st["Q"][0, :n][idx])
                        if q is not None:
                            slot.minq[s] = min(slot.minq[s], q)
                            if q < np.float32(rs["threshold"]):
                                if slot.playon:
                                    slot.would = slot.would or s + 1
                                else:
                                    resigned = True
                if not (stalled or mated or resigned or verdict != RM.NONE):
                    gamma = None if stream[t][0] is None else np.asarray(stream[t][0][g], np.float64)[:len(idx)]
                    j, margin = M.choose_ref(visits[idx], temperature, gamma, eps, float(stream[t][1][g]))
                    mv = int(labels[idx[j]])
                    if f < O.NLABELS:
                        mv = f
                    else:
                        margins.append(margin)
                    if ply < max_plies:
                        recs.append(XS._record(b, s, labels[idx], visits[idx], ply))
                    movers.append(s)
                    ply += 1
                    stalled = mv not in set(int(x) for x in labels)      # BAD_ADVANCE: a forced label that is no root child
                    S.advance(np.array([mv], np.uint16))
                    b, _, r = S.root_state()
                    b, r = b[0], int(r[0])
                o = XS.adjudicate_xq_ref(verdict, mated or resigned, s, b, r, ply, movers, max_plies, stalled)
                if o is None:
                    continue
                if cause == CM.CAUSE_CHASE:
                    o.how = "chase"
                if resigned:
                    o.how = "resign"
                    counters["resigned"] += 1
                o.playon, o.would, o.game_no = (False, 0, 0) if slot is None else (slot.playon, slot.would, slot.game_no)
                if slot is not None and slot.playon and o.result != "stalled":
                    loser = {"red": M.BLACK, "black": M.RED}.get(o.result, -1)
                    counters["playon_games"] += 1
                    if slot.would:
                        counters["playon_would_resign"] += 1
                        if loser != slot.would - 1:
                            counters["playon_false_positives"] += 1
                    for sd in (0, 1):
                        if loser != sd and slot.minq[sd] < 2:
                            hist[hist_bin(slot.minq[sd])] += 1
                out = np.stack(recs[:o.fin_n]) if o.fin_n else np.zeros((0, REC_BYTES), np.uint8)
                out[:, REC_Z] = o.z.astype(np.int8).view(np.uint8)
                finished.append((t, g, o, out))
                if not continuous:
                    active[g] = False
                    break
                S.reset(*start)                     # the slot's next game
                recs, movers, ply = [], [], 0
                history = RR.History(level, fold)
                if slot is not None:
                    slot.game_no += 1
                    slot.fresh(rs)
        finally:
            S.close()
        game_nos[g] = 0 if slot is None else slot.game_no
    finished.sort(key=lambda x: (x[0], x[1]))
    outcomes = [(t, g, o) for t, g, o, _ in finished]
    stats = M.stats_ref([o for _, _, o in outcomes])
    for k, how in (("mates", "mate"), ("repetitions", "repetition"), ("perpetuals", "perpetual"), ("chases", "chase")):
        stats[k] = sum(1 for _, _, o in outcomes if o.how == how)
    records = np.concatenate([x for _, _, _, x in finished]) if finished else np.zeros((0, REC_BYTES), np.uint8)
    return dict(records=records, outcomes=outcomes, stats=stats, resign_stats=counters, hist=hist, active=active,
                min_margin=min(margins) if margins else float("inf"), game_no=game_nos)


# ---- the self-play fixture -----------------------------------------------------------------------------------------------------
# 8 slots on repetition_cases.cpu_openings(8, 4, 13), pos/11 at 16 playouts, 48 lock-step plies at temperature 0.25 with Dirichlet
# noise from numpy stream 3, max_plies 40; resignation at -0.125 from ply 0, 30 % of the games play on, drawn from seed 148
SP = dict(G=8, T=48, playouts=16, max_plies=40, temperature=0.25, eps=0.25, openings=13, stream=3,
          resign=dict(threshold=-0.125, min_ply=0, playon=0.3, seed=148))
LEVELS = {"capture": dict(rules="capture", fold=0, chase=False), "xiangqi": dict(rules="xiangqi", fold=3, chase=True)}


def sp_openings():
    import repetition_cases as RC
    return RC.cpu_openings(SP["G"], 4, SP["openings"])


def sp_stream():
    """stream[t] = (gamma f32 [G, 128], u f32 [G]) for SelfPlay.step_ply(rand=...)."""
    rng = np.random.default_rng(SP["stream"])
    return [(rng.standard_gamma(0.3, (SP["G"], 128)).astype(np.float32), rng.random(SP["G"]).astype(np.float32)) for _ in range(SP["T"])]


@functools.lru_cache(maxsize=None)
def sp_model(level, continuous=True, playon=None, off=False, retune_at=None, retune_to=None):
    """The fixture's games on the CPU oracle, once per process and setting; read-only.  playon: another play-on fraction; off: no
    resignation at all; retune_at / retune_to: the threshold becomes retune_to before step retune_at."""
    boards, side = sp_openings()
    resign = None if off else dict(SP["resign"], **({} if playon is None else dict(playon=playon)))
    return play_selfplay(fakenet.make_forward("pos", 11), SP["playouts"], boards, side, None, sp_stream(), continuous=continuous,
                         max_plies=SP["max_plies"], temperature=SP["temperature"], eps=SP["eps"], resign=resign,
                         retune=None if retune_at is None else {retune_at: retune_to}, **LEVELS[level])


def sp_mix(out):
    """-> dict(resigned, colours: the sides that resigned, crossed_and_lost, false_positives, old_way: games that ended without
    resignation and without a crossing) of a play_selfplay result."""
    oc = [o for _, _, o in out["outcomes"]]
    loser = lambda o: {"red": M.BLACK, "black": M.RED}.get(o.result, -1)
    res = [o for o in oc if o.how == "resign"]
    return dict(resigned=len(res), colours=sorted({loser(o) for o in res}),
                crossed_and_lost=sum(1 for o in oc if o.playon and o.would and loser(o) == o.would - 1),
                false_positives=sum(1 for o in oc if o.playon and o.would and loser(o) != o.would - 1 and o.result != "stalled"),
                old_way=sum(1 for o in oc if o.how != "resign" and not o.would and o.result != "stalled"))
