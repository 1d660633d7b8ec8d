"""Batched, device-resident self-play on top of the lock-step search engine (rows a17-a18 of SURVEY §8).

Mirrors, for G games at once, cchess_main.get_action (main.py:1332-1358) and cchess_main.selfplay
(main.py:1493-1554) of the reference:
  * pi = softmax(log(N)/temperature) over the root children (temperature 1 -> N / sum N),
  * the played move is sampled from 0.75*pi + 0.25*Dirichlet(0.3) when exploring (main.py:1346),
  * every ply records (canonical state, pi scattered over the 2086 labels in canonical orientation —
    rank-flipped for black, main.py:1507-1512 — and the mover),
  * a game ends when a king is captured (z = +1 for the winner's plies, -1 for the loser's) or after
    60 plies without capture (z = 0), main.py:1532-1545.
With rules="xiangqi" (cz_selfplay_set_rules / cz_selfplay_set_repetition, as arena.Match) the games are Xiangqi: pi and the
played move are over the king-safe root children only, a mover without one is mated, and with repetition=N the N-th occurrence
of a position ends the game — the rules act at the root, the search below it stays the reference's.
With resign=X (cz_selfplay_set_resign; the reference plays every game out) a mover whose root value is below X resigns, and a
share of the games plays on to measure how often that would have been wrong (suggest_resign_threshold).
All of it runs on the device (cz_selfplay_choose / cz_search_advance / cz_selfplay_adjudicate / cz_selfplay_flush,
csrc/cz_selfplay.hip): there is no per-ply host synchronisation and no per-game Python loop; finished games hand their
records to a device ring and — in continuous mode — their slot starts the next game at once, so the device stays full
for as long as the loop runs.  The host only drains the ring (drain()).  With several GPUs every rank plays its own
games and only the drained records are exchanged (parallel.py).

Records are packed (include/cchess_hip.h CZ_REC_*: board, mover, <=128 (label, visit count) pairs, z); `to_dense`
expands them to the reference's training tuples (planes [9,10,14] f32, pi [2086], z).  pi is recomputed from the
visit counts with the reference's own float64 expression, so it is bit-identical to what get_action returns.
"""
import numpy as np
import torch

from ._lib import (MAXMOVES, NLABELS, NSQ, REC_BYTES, REC_COUNT, REC_FLAGS, REC_LABELS, REC_PLY, REC_SIDE, REC_VISITS, REC_Z,
                   SP_AVOID_STATS, SP_CHASE_STATS, SP_RESIGN_STATS, SP_RULES_STATS, SP_STATS, SP_TABLEBASE_STATS, out_pointers, tables)
from .rules import RULES, check_rule_options, root_rules_chase_history, root_rules_history, set_rule_options, tablebase_set

REC_MAXMOVES = MAXMOVES
# SelfPlay.stats(): (getter, the names of what it copies out, whether the loop reports them, the getter's further arguments)
STATS_GETTERS = (("cz_selfplay_stats", SP_STATS, lambda sp: True, ()),
                 ("cz_selfplay_rules_stats", SP_RULES_STATS, lambda sp: RULES[sp.rules] != 0, ()),
                 ("cz_selfplay_chase_stats", SP_CHASE_STATS, lambda sp: sp.chase, ()),
                 ("cz_selfplay_avoid_stats", SP_AVOID_STATS, lambda sp: sp.avoid, ()),
                 ("cz_selfplay_resign_stats", SP_RESIGN_STATS, lambda sp: sp._resign_on, (None,)),
                 ("cz_selfplay_tablebase_stats", SP_TABLEBASE_STATS, lambda sp: sp._tb_on, ()))


def pack_records(boards, side, labels, visits, counts, z, ply=None):
    """-> uint8 [n, REC_BYTES].  boards u8 [n,90]; labels u16 [n,128]; visits [n,128] ints; counts; z in {-1,0,1}."""
    n = boards.shape[0]
    rec = np.zeros((n, REC_BYTES), np.uint8)
    rec[:, :NSQ] = boards
    rec[:, REC_SIDE] = side
    rec[:, REC_COUNT] = counts
    rec[:, REC_Z] = np.asarray(z, np.int8).view(np.uint8)
    v = np.asarray(visits, np.int64)
    rec[:, REC_FLAGS] = (v > 65535).any(axis=1)
    if ply is not None:
        rec[:, REC_PLY:REC_PLY + 2] = np.ascontiguousarray(ply, np.uint16).view(np.uint8).reshape(n, 2)
    rec[:, REC_LABELS:REC_LABELS + 256] = np.ascontiguousarray(labels, np.uint16).view(np.uint8).reshape(n, 256)
    rec[:, REC_VISITS:REC_VISITS + 256] = np.ascontiguousarray(np.minimum(v, 65535), np.uint16).view(np.uint8).reshape(n, 256)
    return rec


def unpack_records(rec):
    rec = np.ascontiguousarray(rec, np.uint8).reshape(-1, REC_BYTES)
    n = rec.shape[0]
    return dict(boards=rec[:, :NSQ].copy(), side=rec[:, REC_SIDE].copy(), counts=rec[:, REC_COUNT].copy(),
                z=rec[:, REC_Z].copy().view(np.int8), flags=rec[:, REC_FLAGS].copy(),
                ply=rec[:, REC_PLY:REC_PLY + 2].copy().view(np.uint16).reshape(n),
                labels=rec[:, REC_LABELS:REC_LABELS + 256].copy().view(np.uint16).reshape(n, 128),
                visits=rec[:, REC_VISITS:REC_VISITS + 256].copy().view(np.uint16).reshape(n, 128))


def canonical_boards(boards, side):
    """try_flip (main.py:560-574) on piece-code boards: for black reverse the rank order and swap the colours."""
    boards = np.asarray(boards, np.uint8).reshape(-1, NSQ)
    n = boards.shape[0]
    b = boards.reshape(n, 10, 9)
    flip = np.asarray(side).astype(bool)
    fb = b[:, ::-1, :]
    fb = np.where(fb == 0, 0, np.where(fb > 7, fb - 7, fb + 7)).astype(np.uint8)
    return np.where(flip[:, None, None], fb, b).reshape(n, NSQ)


def canonical_planes(boards, side):
    """generate_inputs (main.py:531-557) on the host for record expansion: [n,9,10,14] f32 with quirk Q1."""
    canon = canonical_boards(boards, side)
    n = canon.shape[0]
    planes = np.zeros((n, 9, 10, 14), np.float32)
    cells = (np.arange(9)[:, None] * 9 + np.arange(10)[None, :])  # the reference's 9-stride read (quirk Q1)
    code = canon[:, cells]  # [n,9,10]
    for c in range(14):
        planes[..., c] = (code == c + 1)
    return planes


def visit_policy(visits, temperature=1.0):
    """get_action's probs (main.py:1341, softmax :1111-1116) with the reference's own float64 expression:
    softmax(1.0 / temperature * np.log(visits)); zero visits -> log 0 = -inf -> probability 0.  No visit at all — under
    rules="xiangqi" every simulation of a search can go to children that are not king-safe and so are not in the record — is
    1 / k for each, what the choose kernel played from (wave_visit_policy; the reference's expression is NaN there)."""
    visits = np.asarray(visits, dtype=np.int64)
    if not visits.any():
        return np.full(len(visits), 1.0 / len(visits))
    with np.errstate(divide="ignore"):
        x = 1.0 / temperature * np.log(visits)
    probs = np.exp(x - np.max(x))
    probs /= np.sum(probs)
    return probs


def to_dense(rec, temperature=1.0, exact=True):
    """Packed records -> (planes [n,9,10,14] f32, pi [n,2086] f64, z [n] f32): the tuples cchess_main.run extends
    data_buffer with (main.py:1234-1240).  exact: pi through visit_policy record by record (bit-identical to the
    reference); otherwise one vectorised pass (same values to the last ulp or two)."""
    u = unpack_records(rec)
    n = len(u["side"])
    unflip = tables()["unflip"].astype(np.int64)
    pi = np.zeros((n, NLABELS), np.float64)
    if exact:
        for i in range(n):
            k = int(u["counts"][i])
            if k == 0:
                continue
            lab = u["labels"][i, :k].astype(np.int64)
            if u["side"][i]:
                lab = unflip[lab]  # rank-flipped labels for black, main.py:1507-1512
            pi[i, lab] = visit_policy(u["visits"][i, :k], temperature)
    elif n:
        k = u["counts"].astype(np.int64)
        valid = np.arange(128)[None, :] < k[:, None]
        with np.errstate(divide="ignore"):
            x = np.where(valid, np.log(u["visits"].astype(np.float64)) / temperature, -np.inf)
        x = np.where(valid & ~u["visits"].any(axis=1, keepdims=True), 0.0, x)   # no visit at all: 1 / k each, as visit_policy
        e = np.exp(x - x.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
        lab = u["labels"].astype(np.int64)
        lab = np.where(valid, lab, 0)
        lab = np.where(u["side"][:, None].astype(bool), unflip[lab], lab)
        rows = np.repeat(np.arange(n), 128).reshape(n, 128)
        pi[rows[valid], lab[valid]] = p[valid]
    return canonical_planes(u["boards"], u["side"]), pi, u["z"].astype(np.float32)


def suggest_resign_threshold(hist, target_fp, min_samples=100):
    """The resignation threshold that the play-on games' histogram (SelfPlay.resign_histogram: the lowest root value of every
    side that did not lose its play-on game, 64 bins of 1/32 over [-1, 1)) allows at a false-positive rate of target_fp: the
    largest bin edge e = -1 + b / 32, b in 0..64, with sum(hist[:b]) / sum(hist) <= target_fp — a side resigns below the
    threshold, and the edges are exact in float32, so the entries below e are the bins < b (the kernel rounds q + 1 to float32
    before it bins: a value within one rounding step below an edge counts in the bin above it).  None below min_samples
    entries (too few play-on games to say)."""
    hist = np.asarray(hist, np.int64).reshape(64)
    total = int(hist.sum())
    if total < max(int(min_samples), 1):
        return None
    below = np.concatenate([[0], np.cumsum(hist)])            # below[b] = entries in the bins < b
    ok = np.nonzero(below / total <= float(target_fp))[0]
    return -1.0 + int(ok[-1]) / 32.0 if len(ok) else None


class SelfPlay:
    """G concurrent self-play games on one GPU, device-resident.

    continuous=True : a finished game's slot starts a new game at once (the production loop: the batch never decays);
    continuous=False: finished games are parked — play() returns when every game has ended (one game per slot).
    rules: "capture" — the reference's games: pseudo-legal moves, a game ends when a king is taken; "xiangqi" — the move is
    chosen and recorded among the king-safe root children, and a mover without one loses (checkmate or stalemate).
    repetition (rules="xiangqi" only): 0 — no repetition rule; 2..8 — a game ends when its position occurs for that many times
    since the last capture: a draw, or a loss for the side that alone checked with every move of the cycle.
    chase (with a repetition fold only): True — when neither side checked so, a side that alone chased one and the same
    unprotected piece with every move of the cycle has lost (cz_selfplay_set_chase, as arena.Match(chase=True)); z as for
    perpetual check.
    resign: None — every game is played out; a value — from ply resign_min_ply on, a mover whose root value (the Q of its most
    visited candidate child) is below it resigns (cz_selfplay_set_resign), except in the games that play on: a share
    resign_playon of the games, drawn from `seed` per slot and game, never resigns and is counted instead — stats() says how many
    of them crossed the threshold and how many of those did not lose (the false positives), resign_histogram() what threshold
    a false-positive rate allows (suggest_resign_threshold).
    tablebase (rules="xiangqi" only): None — games are played out; a tablebase.Tablebase (all its loaded tables) or a
    tablebase.DeviceSet — a game whose position after a move is in one of the tables ends there with the table's result
    (cz_selfplay_set_tablebase): z as for a king capture, counted in the wins / draws and in stats()["tablebase"].  A game
    that starts in a covered position plays one ply first; set_tablebase() attaches or detaches between two plies.
    """

    def __init__(self, engine, net, playouts, exploration=True, temperature=1.0, seed=0, max_plies=512, ring_records=None,
                 continuous=True, eval_cache=False, xcache_log2=0, rules="capture", repetition=0, chase=False, resign=None,
                 resign_min_ply=0, resign_playon=0.1, tablebase=None, avoid_repetition=False):
        check_rule_options("SelfPlay", rules, repetition, chase, tablebase, resign_min_ply, resign_playon, avoid=avoid_repetition)
        self.avoid = bool(avoid_repetition)   # the mover does not choose a move that loses by repetition (cz_selfplay_set_avoid)
        self.tablebase = tablebase
        self._tb_set = self._tb_own = None
        self.resign = None if resign is None else float(resign)
        self.resign_min_ply = int(resign_min_ply)
        self.resign_playon = float(resign_playon)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.rules = rules
        self.repetition = int(repetition)
        self.chase = bool(chase)
        self.eng, self.net = engine, net
        self.playouts = int(playouts)
        self.exploration = bool(exploration)
        self.temperature = float(temperature)
        self.max_plies = int(max_plies)
        self.continuous = bool(continuous)
        # evaluation cache (engine.set_eval_cache): valid as long as the net's weights do not change — start() empties it
        self.eval_cache = bool(eval_cache)
        # its cross-tree level (engine.set_xcache): games from one start position share their openings
        self.xcache_log2 = int(xcache_log2) if eval_cache else 0
        self.dev = engine.dev
        self.gen = torch.Generator(device=self.dev).manual_seed(seed)
        self.ring_records = ring_records
        self.plies = 0
        self.lock_steps = 0
        if engine.width != 1:
            raise ValueError("SelfPlay drives one simulation in flight per tree (thousands of trees fill the net batch)")

    # -- setup -------------------------------------------------------------------------------------
    def start(self, boards, side, rr=None):
        """Fresh trees on the given positions; every later game of a slot starts from the same position."""
        eng = self.eng
        if self.eval_cache or eng.eval_cache:
            eng.set_eval_cache(self.eval_cache)   # turning it on empties it: new weights, new cache
            if self.eval_cache and (self.xcache_log2 or eng.xcache_log2):
                eng.set_xcache(self.xcache_log2)
        eng.reset(boards, side, rr)
        eng.compact = not self.continuous   # parked games drop out of the net's batch; a full batch needs no compaction
        G = eng.G
        eng.ctx.call("cz_selfplay_begin", self.max_plies, None, None, None)
        set_rule_options("cz_selfplay", eng.ctx.h, self.rules, self.repetition, self.chase, self.avoid)
        self._resign_on = self.resign is not None
        self._apply_resign()
        self._tb_on = False   # cz_selfplay_begin detached whatever was attached
        self.set_tablebase(self.tablebase)
        self._active_ptr, = out_pointers("cz_selfplay_active", eng.ctx.h, 1)
        R = int(self.ring_records or max(65536, 64 * G))
        self.ring = torch.zeros((R, REC_BYTES), dtype=torch.uint8, device=self.dev)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.dev)       # records ever handed to the ring
        self.read_cursor = torch.zeros(1, dtype=torch.int64, device=self.dev)  # records the host has drained
        self._read = 0
        self.played = torch.empty(G, dtype=torch.int16, device=self.dev)
        self.fin_n = torch.zeros(G, dtype=torch.int32, device=self.dev)
        self._alpha = torch.full((G, MAXMOVES), 0.3, dtype=torch.float32, device=self.dev)
        # what the getters copy out: cz_selfplay_stats' at the front (drain_device), the others' behind as stats() asks, then the histogram
        self._stats = torch.zeros(sum(len(names) for _, names, _, _ in STATS_GETTERS) + 64, dtype=torch.int64, device=self.dev)
        self.plies = 0
        self.lock_steps = 0
        self._dropped_seen = 0
        self.overflow_intervals = 0

    def _apply_resign(self):
        if self._resign_on:
            self.eng.ctx.call("cz_selfplay_set_resign", float("nan") if self.resign is None else self.resign, self.resign_min_ply,
                              self.resign_playon, self.seed)

    def set_tablebase(self, tablebase):
        """Attaches a Tablebase / DeviceSet to a started loop, or detaches it (None) — between any two plies.  A DeviceSet made
        here from a Tablebase is closed when it is replaced and by close()."""
        check_rule_options("SelfPlay", self.rules, self.repetition, self.chase, tablebase)
        dset, own = tablebase_set(tablebase)
        self.eng.ctx.call("cz_selfplay_set_tablebase", None if dset is None else dset.h)
        if self._tb_own is not None:
            self._tb_own.close()
        self.tablebase, self._tb_set, self._tb_own = tablebase, dset, own
        self._tb_on = self._tb_on or dset is not None

    def close(self):
        """Detaches the table set (a started loop holds it) and closes the one this loop made itself"""
        if self._tb_set is not None:
            self.set_tablebase(None)

    def set_resign_threshold(self, threshold):
        """Retunes the resignation threshold of a started loop (None: no ply is judged until the next call): the games in
        progress, their play-on draws and the counters stay.  On a loop started without resignation this switches it on."""
        self.resign = None if threshold is None else float(threshold)
        self._resign_on = self._resign_on or self.resign is not None
        self._apply_resign()

    # -- one ply of every game ------------------------------------------------------------------------
    def step_ply(self, forward=None, forced=None, rand=None):
        """Search, choose, record, advance, adjudicate, flush — all enqueued, nothing synchronised.
        forced: int16/uint16 [G] labels overriding the sampled moves (0xFFFF = sample), for replaying recorded games.
        rand: (gamma [G,128], u [G]) to sample with instead of random_inputs() (replaying a recorded random stream)."""
        eng = self.eng
        fwd = forward or self.net.forward_device
        eng.search(fwd, self.playouts, active=None if self.continuous else self._active_ptr)
        self._transition(0, forced, rand)
        self.plies += 1

    def random_inputs(self):
        """The random numbers of one cz_selfplay_choose, drawn from self.gen: (gamma f32 [G,128] Gamma(0.3, 1) variates —
        normalised over a game's k children they are np.random.dirichlet(0.3 * ones(k)), main.py:1346 — or None when not
        exploring, u f32 [G] uniforms in [0, 1) for the inverse-CDF pick of np.random.choice)."""
        gamma = None
        if self.exploration:
            gamma = torch._standard_gamma(self._alpha, generator=self.gen)
        u = torch.rand(self.eng.G, generator=self.gen, device=self.dev, dtype=torch.float32)
        return gamma, u

    def _transition(self, min_sims, forced=None, rand=None):
        """choose / advance / adjudicate / flush for every game (min_sims = 0) or for the games whose search has completed
        min_sims simulations (asynchronous plies).  rand: (gamma, u) replacing random_inputs() (gamma may be None)."""
        eng, ctx = self.eng, self.eng.ctx
        if rand is None:
            gamma, u = self.random_inputs()
        else:
            gamma, u = ctx.tensor(rand[0], torch.float32), ctx.tensor(rand[1], torch.float32)
            assert (gamma is None or gamma.shape == (eng.G, MAXMOVES)) and u.shape == (eng.G,)
        f = ctx.tensor(forced, torch.int16)
        ctx.call("cz_selfplay_choose", gamma, u, f, self.temperature, 0.25 if self.exploration else 0.0, int(min_sims), self.played)
        eng.advance(self.played)
        ctx.call("cz_selfplay_adjudicate", 1 if self.continuous else 0, self.played if min_sims > 0 else None, self.fin_n)
        csum = torch.cumsum(self.fin_n, 0, dtype=torch.int64)
        offset = csum - self.fin_n + self.cursor
        ctx.call("cz_selfplay_flush", self.fin_n, offset, self.ring, self.ring.shape[0], self.read_cursor)
        self.cursor += csum[-1:]

    def run(self, plies, forward=None):
        for _ in range(int(plies)):
            self.step_ply(forward)

    def run_async(self, steps, forward=None, every=8, terminal_extra=4):
        """ASYNCHRONOUS plies (continuous mode): `steps` lock-steps of the net, every game at its own pace.  Each step is
        one select / net / expand for all slots; every `every` steps the games whose search has completed its `playouts`
        simulations choose, move, are adjudicated and — if finished — re-seeded.  With terminal_extra > 0 simulations
        that end on terminal / drawn leaves complete inside the select launch without a net row, so a game finishes its
        search in fewer steps than it has playouts and the net batch is never spent on leaves that need no evaluation.
        Per tree the simulations are the same sequence as in lock-step plies (trees bit-identical for the same evaluations)."""
        assert self.continuous, "asynchronous plies re-seed finished slots at once"
        eng = self.eng
        fwd = forward or self.net.forward_device
        prev_extra = eng.terminal_extra
        eng.set_terminal_extra(terminal_extra)
        eng.set_sim_target(self.playouts)
        try:
            for i in range(int(steps)):
                eng.step(fwd, mode=1)            # an unexpanded root (fresh game, new ply) is expanded by this step
                self.lock_steps += 1
                if (i + 1) % every == 0:
                    self._transition(self.playouts)
        finally:
            eng.set_sim_target(0)
            eng.set_terminal_extra(prev_extra)

    def play(self, forward=None, max_plies=None):
        """continuous=False: play until every game has ended (or max_plies plies); returns the drained records.
        continuous=True needs max_plies (the loop never runs out of games)."""
        if self.continuous and max_plies is None:
            raise ValueError("a continuous self-play loop has no natural end: pass max_plies (or drive step_ply / drain yourself)")
        n = 0
        out = []
        while max_plies is None or n < max_plies:
            self.step_ply(forward)
            n += 1
            if n % 8 == 0 or (max_plies is not None and n >= max_plies):
                out.append(self.drain())
                if not self.continuous and not bool(self.active().any().item()):
                    break
        out.append(self.drain())
        return np.concatenate(out, axis=0) if out else np.zeros((0, REC_BYTES), np.uint8)

    # -- host side --------------------------------------------------------------------------------------
    def active(self):
        """uint8 [G] host tensor: 1 = game in progress (synchronises)."""
        return torch.from_numpy(self.eng.ctx.download(self._active_ptr, np.uint8, self.eng.G))

    def history(self):
        """(keys u64 [G, 64], checks u8 [G, 64]) on the host: the slots' position rings (cz_selfplay_history; repetition != 0),
        position i of a slot's game at [i & 63]."""
        return root_rules_history("cz_selfplay", self.eng.ctx.h, self.eng.ctx, self.eng.G)

    def chase_history(self):
        """chase u64 [G, 64, 4] on the host: the slots' rings of chase records (cz_selfplay_chase_history; chase=True)."""
        return root_rules_chase_history("cz_selfplay", self.eng.ctx.h, self.eng.ctx, self.eng.G)

    def drain_device(self, on_overflow="raise"):
        """-> uint8 [n, REC_BYTES] DEVICE tensor with the records finished since the last drain (synchronises on the
        cursor and the drop counter).  The returned rows stay valid until the ring wraps over them.
        If finished games have been DROPPED since the last drain because the ring was full of undrained rows
        (cz_selfplay_flush skips such a game but the cursor still advances by its length, so the interval contains slots
        that were never written), the whole interval is discarded — never handed out — and, with on_overflow = "raise"
        (default), a RuntimeError says so; on_overflow = "skip" counts it in self.overflow_intervals and returns no rows
        (a long training run prefers losing one interval of samples to stopping).  Drain more often or pass a larger
        ring_records to avoid it."""
        self.eng.ctx.call("cz_selfplay_stats", self._stats)
        dropped = int(self._stats[SP_STATS.index("dropped")].item())
        c = int(self.cursor.item())
        if dropped > self._dropped_seen:
            n_new = dropped - self._dropped_seen
            self._dropped_seen = dropped
            self._read = c
            self.read_cursor.fill_(c)
            self.overflow_intervals += 1
            msg = ("self-play record ring overflow: %d records of finished games were dropped since the last drain "
                   "(ring of %d records; drain more often or raise ring_records); the interval's records are discarded"
                   % (n_new, self.ring.shape[0]))
            if on_overflow == "raise":
                raise RuntimeError(msg)
            print("WARNING:", msg)
            return self.ring[:0]
        r, R = self._read, self.ring.shape[0]
        n = min(c - r, R)
        if n <= 0:
            return self.ring[:0]
        lo = (c - n) % R
        out = self.ring[lo:lo + n] if lo + n <= R else torch.cat([self.ring[lo:], self.ring[:lo + n - R]], 0)
        self._read = c
        self.read_cursor.fill_(c)
        return out

    def drain(self):
        """-> uint8 [n, REC_BYTES] host array of the records finished since the last drain."""
        return self.drain_device().cpu().numpy().reshape(-1, REC_BYTES)

    def stats(self):
        """Running totals since start(): games, red_wins, black_wins, draws, plies (records), stalled, dropped, sims; with
        rules="xiangqi" also mates, repetitions, perpetuals — the games among them that ended by mate (a win), by a repetition
        draw, by perpetual check (a win); with chase=True also chases — the games that ended by perpetual chase (a win; not
        among the perpetuals); with resignation on also resigned, playon_games, playon_would_resign, playon_false_positives —
        the games a mover resigned (a win for the other side), the play-on games finished, those in which a side crossed the
        threshold, and those of them that side won or drew; with a table set attached at any time since start() also tablebase —
        the games adjudicated from a table (counted among the wins / draws too)."""
        keys = []
        for getter, names, on, extra in STATS_GETTERS:
            if on(self):
                self.eng.ctx.call(getter, self._stats[len(keys):], *extra)
                keys += names
        d = {k: int(v) for k, v in zip(keys, self._stats.cpu().numpy())}
        d["sims"] += int(self.eng.status()[2].sum().item())   # + the simulations of the searches in progress
        d["plies_played"] = self.plies          # lock-step plies (step_ply)
        d["lock_steps"] = self.lock_steps       # select / net / expand steps of the asynchronous loop (run_async)
        return d

    def resign_histogram(self):
        """int64 [64] on the host: the lowest root value of every side that did not lose its play-on game, in bins of 1 / 32 over
        [-1, 1) (cz_selfplay_resign_stats; all zero without resignation) — the input of suggest_resign_threshold."""
        self.eng.ctx.call("cz_selfplay_resign_stats", self._stats[-64 - len(SP_RESIGN_STATS):], self._stats[-64:])
        return self._stats[-64:].cpu().numpy().copy()
