"""Evaluation matches between two players on the GPU: the reference's policy_evaluate (main.py:1207-1222, commented out there).

A match is G concurrent games between player A and player B.  Each player has its own search engine (its own trees, its
own net and its own playout budget); slot g of both engines belongs to the same game.  The per-ply bookkeeping runs on
the device (csrc/cz_match.hip): the mover's move on the mover's tree, both trees follow it (the opponent keeps its subtree
for the move, update_tree after the opponent's move, main.py:272-276), check_end (:1380-1392), the result, and the slot's
next game from a queue of 2 x n_openings games — game i plays opening i // 2 with A red when i is even.  The host reads
one counter every few plies to know when every game has ended.

    res = Match((net_a, 400), (net_b, 400), random_openings(512, 4, seed=1), slots=1024).play()
    res.score, res.elo, res.elo_95

A player is (net_or_forward, playouts): a PolicyValueNet (the fused search path), a policy_value_network, or a plain
forward(planes) -> (logits, value) callable on device tensors (tests).  With several ranks (torch.distributed), opening pair
p is played on rank p % world and every rank returns the same MatchResult.
"""
import argparse
import contextlib
import ctypes as C
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

from ._lib import (MATCH_ABORTED, MATCH_CHASE, MATCH_KING, MATCH_MATE, MATCH_PERPETUAL, MATCH_PLY_CAP, MATCH_REPETITION, MATCH_RESIGN, MATCH_RR60, MATCH_TABLEBASE, NSQ, call,
                   lib, out_pointers, tables)
from .engine import SearchEngine, plane_format, pool_nodes
from .notation import player_to_side, state_to_board
from .rules import (RULES, add_rule_flags, check_rule_flags, check_rule_options, root_rules_chase_history, root_rules_history,   # noqa: F401 (RULES: re-exported)
                    set_rule_options, tablebase_set)

REASONS = {0: "unfinished", MATCH_KING: "king", MATCH_RR60: "rr60", MATCH_PLY_CAP: "ply_cap", MATCH_ABORTED: "aborted", MATCH_MATE: "mate",
           MATCH_REPETITION: "repetition", MATCH_PERPETUAL: "perpetual", MATCH_CHASE: "chase", MATCH_RESIGN: "resign", MATCH_TABLEBASE: "tablebase"}


def is_scored(reason, resign=False, tablebase=False):
    """A finished game that counts: every ending but "aborted" (a mate, rules="xiangqi", is a loss for the mated side; with
    repetition != 0 a repetition is a draw and a perpetual check a loss for the checking side; with chase a perpetual chase is
    a loss for the chasing side).  resign: the match was played with resignation (Match(resign=...)) — then, and only then, a
    game can end as "resign", a loss for the side that resigned, and counts; in a match without it no game carries that reason
    and the code counts no more than an unassigned one.  tablebase: the match was played with a table set (Match(tablebase=...))
    — the same for "tablebase", the table's result of the position a game reached."""
    reason = np.asarray(reason, np.int64)
    scored = ((reason >= MATCH_KING) & (reason <= MATCH_PLY_CAP)) | ((reason >= MATCH_MATE) & (reason <= MATCH_PERPETUAL)) | (reason == MATCH_CHASE)
    if resign:
        scored = scored | (reason == MATCH_RESIGN)
    if tablebase:
        scored = scored | (reason == MATCH_TABLEBASE)
    return scored


# ---- openings ------------------------------------------------------------------------------------------------------------
class Openings:
    """n start positions: boards u8 [n, 90], side u8 [n], rr i32 [n], keys u64 [n] (Zobrist, cz_hash), moves: the labels
    that lead to each from the start position (empty for user positions)."""

    def __init__(self, boards, side, rr=None, moves=None, keys=None):
        self.boards = np.ascontiguousarray(boards, np.uint8).reshape(-1, NSQ)
        n = self.boards.shape[0]
        self.side = np.ascontiguousarray(side, np.uint8).reshape(n)
        self.rr = np.zeros(n, np.int32) if rr is None else np.ascontiguousarray(rr, np.int32).reshape(n)
        self.moves = [list(m) for m in moves] if moves is not None else [[] for _ in range(n)]
        self.keys = None if keys is None else np.ascontiguousarray(keys, np.uint64).reshape(n)

    def __len__(self):
        return self.boards.shape[0]

    def subset(self, idx):
        idx = np.asarray(idx, np.int64)
        return Openings(self.boards[idx], self.side[idx], self.rr[idx], [self.moves[i] for i in idx],
                        None if self.keys is None else self.keys[idx])


def openings_from_states(states):
    """User openings: each a state string (red to move), or (state, player 'w' / 'b'[, restrict_round])."""
    boards, side, rr = [], [], []
    for s in states:
        if isinstance(s, str):
            s = (s, "w")
        boards.append(state_to_board(s[0]))
        side.append(player_to_side(s[1]))
        rr.append(int(s[2]) if len(s) > 2 else 0)
    return Openings(np.stack(boards), side, rr)


def random_openings(n, plies, seed, device=None):
    """n distinct positions (distinct by Zobrist key, side to move included) after `plies` uniform random legal plies from
    the start position, both kings on the board, generated on the GPU with the rules kernels (movegen -> uniform pick ->
    apply_move -> hash).  A line that captures a king or meets a position without a legal move is dropped.  The same
    seed gives the same set, in the same order."""
    from .rules import START_BOARD, Rules
    n, plies = int(n), int(plies)
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    rules = Rules(device=dev.index)
    gen = torch.Generator(device=dev).manual_seed(int(seed))
    out_b, out_s, out_r, out_m, out_k, seen = [], [], [], [], [], set()
    for _ in range(64):
        if len(out_k) >= n:
            break
        M = max(256, 2 * (n - len(out_k)))
        boards = torch.from_numpy(np.tile(START_BOARD, (M, 1))).to(dev)
        side = torch.zeros(M, dtype=torch.uint8, device=dev)
        rr = torch.zeros(M, dtype=torch.int32, device=dev)
        ok = torch.ones(M, dtype=torch.bool, device=dev)
        labels = torch.zeros((M, plies), dtype=torch.int64, device=dev)
        for ply in range(plies):
            moves, count, _ = rules.movegen(boards, side, want_mask=False, strict=True)
            cnt = count.to(torch.int64) & 0xFFFF
            ok &= cnt > 0
            r = (torch.rand(M, generator=gen, device=dev) * cnt.clamp(min=1)).to(torch.int64).clamp(max=127)
            lab = moves.gather(1, torch.minimum(r, (cnt - 1).clamp(min=0)).unsqueeze(1)).squeeze(1)
            lab = torch.where(ok, lab, torch.full_like(lab, -1))
            cap, term = rules.apply_move(boards, side, lab)
            ok &= term == 0
            rr = torch.where(cap != 0, torch.zeros_like(rr), rr + 1)
            labels[:, ply] = lab.to(torch.int64) & 0xFFFF
        keys = rules.hash(boards, side).cpu().numpy().view(np.uint64)
        okh, bh, sh, rh, lh = ok.cpu().numpy(), boards.cpu().numpy(), side.cpu().numpy(), rr.cpu().numpy(), labels.cpu().numpy()
        for i in range(M):
            k = int(keys[i])
            if not okh[i] or k in seen:
                continue
            seen.add(k)
            out_b.append(bh[i]); out_s.append(sh[i]); out_r.append(rh[i]); out_m.append([int(x) for x in lh[i]]); out_k.append(k)
            if len(out_k) >= n:
                break
    if len(out_k) < n:
        raise ValueError("random_openings: only %d distinct positions found after %d random plies (asked for %d)" % (len(out_k), plies, n))
    return Openings(np.stack(out_b), out_s, out_r, out_m, np.array(out_k, np.uint64))


def book_openings(book, n, plies, seed, min_games=2):
    """n distinct positions (distinct by Zobrist key, side to move included) `plies` plies into an opening book
    (cchess_zero_amd.book.Book): Book.playout — every move drawn in proportion to its games among the entries of at least min_games —
    over-drawn and de-duplicated, as random_openings does; a line that leaves the book before `plies` is dropped.  The same seed
    gives the same set, in the same order.  ValueError with the count found if the book does not hold n of them."""
    from .rules import Rules
    n, plies = int(n), int(plies)
    gen = torch.Generator(device=book.ctx.device).manual_seed(int(seed))
    rules = Rules(ctx=book.ctx)
    out_b, out_s, out_r, out_m, out_k, seen = [], [], [], [], [], set()
    for _ in range(8):
        if len(out_k) >= n:
            break
        found = len(out_k)
        po = book.playout(max(256, 4 * (n - found)), plies, gen, min_games, book.rules)
        keys = rules.hash(po.boards, po.side).cpu().numpy().view(np.uint64)
        for i in np.nonzero(po.lens == plies)[0]:
            k = int(keys[i])
            if k in seen:
                continue
            seen.add(k)
            out_b.append(po.boards[i]); out_s.append(po.side[i]); out_r.append(po.rr[i]); out_m.append(po.labels[i]); out_k.append(k)
            if len(out_k) >= n:
                break
        if len(out_k) == found:   # a whole over-drawn round without a new position: the book holds no more
            break
    if len(out_k) < n:
        raise ValueError("book_openings: only %d distinct positions found %d plies into the book (asked for %d)" % (len(out_k), plies, n))
    return Openings(np.stack(out_b), out_s, out_r, out_m, np.array(out_k, np.uint64))


def exhaustive_openings(plies, device=None):
    """EVERY distinct position (distinct by Zobrist key, side to move included; the first occurrence in generation order)
    after `plies` king-safe plies from the start position, on the GPU (movegen_kingsafe -> successors, ply by ply, -> hash).
    moves holds the line that led to the first occurrence, rebuilt from the successors' parents and labels.  King-safe moves
    take no king: both kings are on the board by construction.  1 920 openings at 2 plies, under 79 666 at 3."""
    from .rules import START_BOARD, Rules
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    rules = Rules(device=dev.index)
    boards = torch.from_numpy(START_BOARD[None].copy()).to(dev)
    side = torch.zeros(1, dtype=torch.uint8, device=dev)
    rr = torch.zeros(1, dtype=torch.int32, device=dev)
    lines = torch.zeros((1, 0), dtype=torch.int64, device=dev)
    for _ in range(int(plies)):
        mv, cnt, _, _ = rules.movegen_kingsafe(boards, side, want_mask=False, pad=False)
        boards, side, cap, par, label = rules.successors(boards, side, mv, cnt)
        par = par.to(torch.int64)
        rr = torch.where(cap != 0, torch.zeros_like(rr[par]), rr[par] + 1)
        lines = torch.cat([lines[par], (label.to(torch.int64) & 0xFFFF).unsqueeze(1)], 1)
    keys = rules.hash(boards, side).cpu().numpy().view(np.uint64)
    first = np.sort(np.unique(keys, return_index=True)[1])
    return Openings(boards.cpu().numpy()[first], side.cpu().numpy()[first], rr.cpu().numpy()[first],
                    [[int(x) for x in l] for l in lines.cpu().numpy()[first]], keys[first])


def as_openings(openings):
    if isinstance(openings, Openings):
        return openings
    if isinstance(openings, (list, tuple)) and openings and isinstance(openings[0], (str, list, tuple)) and not isinstance(openings[0], np.ndarray):
        return openings_from_states(openings)
    raise TypeError("openings: an Openings (random_openings) or a list of state strings / (state, player[, rr]) tuples")


# ---- scores --------------------------------------------------------------------------------------------------------------
def elo(score):
    """Elo difference of an expected score: -400 log10(1 / s - 1).  None for s <= 0 or s >= 1 (the difference is infinite:
    every scored game lost / won) and for no score at all."""
    if score is None or not (0.0 < score < 1.0):
        return None
    return -400.0 * math.log10(1.0 / score - 1.0)


def pentanomial(result, reason, resign=False, tablebase=False):
    """Counts of the opening pairs' scores for A: index k = points out of 2 times 2 (0, 0.5, 1, 1.5, 2 -> 0..4), over the
    pairs (games 2p, 2p + 1) whose two games were both scored (an aborted game drops its pair); resign, tablebase as is_scored's."""
    result = np.asarray(result, np.int64)
    reason = np.asarray(reason, np.int64)
    scored = is_scored(reason, resign, tablebase)
    pair_ok = scored[0::2] & scored[1::2]
    x = (result[0::2] + 1) + (result[1::2] + 1)          # twice A's points of the pair: 0..4
    return np.bincount(x[pair_ok], minlength=5)[:5].astype(np.int64)


def pentanomial_interval(counts, z=1.959963984540054):
    """(mean score, lo, hi) of the per-game score from the pentanomial counts: the pair score x / 2 has mean s and variance
    sum_k c_k (x_k / 2 - s)^2 / n over the n pairs; s +- z sqrt(var / n).  None without a pair."""
    c = np.asarray(counts, np.float64)
    n = c.sum()
    if n <= 0:
        return None
    xs = np.arange(5) / 4.0                                # pair score per game: 0, 0.25, 0.5, 0.75, 1
    s = float((c * xs).sum() / n)
    var = float((c * (xs - s) ** 2).sum() / n)
    half = z * math.sqrt(var / n)
    return s, s - half, s + half


class MatchResult:
    """Per game (global game index): result (+1 / 0 / -1 for A), a_red, plies, reason (REASONS), moves (ICCS labels).
    W / D / L for A overall and by colour over the scored games (aborted games excluded), score = (W + D / 2) / scored,
    elo and its 95 % interval from the pentanomial distribution of the opening pairs, simulations, seconds, sims_per_s;
    rules ("capture" / "xiangqi") and mates: the games that ended because the mover had no king-safe move; repetition (the
    fold, 0 = no such rule), repetitions: the games drawn by it, perpetuals: the games lost by perpetual check; chase (the
    perpetual-chase rule was on), chases: the games lost by perpetual chase; resign (the threshold the match resigned on, None = games were played
    out), resigns: the games a mover resigned; tablebase (the match was played with a table set), tablebases: the games that
    ended with a table's result."""

    def __init__(self, result, a_red, plies, reason, moves, simulations, seconds, players, rules="capture", repetition=0, chase=False, resign=None,
                 tablebase=False, avoid=False, avoided=0, forced_repetitions=0):
        self.result = np.asarray(result, np.int8)
        self.a_red = np.asarray(a_red, np.uint8)
        self.plies = np.asarray(plies, np.int32)
        self.reason = np.asarray(reason, np.uint8)
        lab = tables()["labels"] if moves is not None else None
        self.moves = [[lab[int(x)] for x in row if x != 0xFFFF] for row in moves] if moves is not None else None
        self.games = len(self.result)
        self.resign = None if resign is None else float(resign)
        self.tablebase = bool(tablebase)
        self.tablebases = int((self.reason == MATCH_TABLEBASE).sum())
        scored = is_scored(self.reason, self.resign is not None, self.tablebase)
        self.rules = rules
        self.mates = int((self.reason == MATCH_MATE).sum())
        self.repetition = int(repetition)
        self.repetitions = int((self.reason == MATCH_REPETITION).sum())
        self.perpetuals = int((self.reason == MATCH_PERPETUAL).sum())
        self.chase = bool(chase)
        self.chases = int((self.reason == MATCH_CHASE).sum())
        # avoid_repetition: the plies at which a move that loses by repetition was taken from the choice / at which every move lost
        self.avoid, self.avoided, self.forced_repetitions = bool(avoid), int(avoided), int(forced_repetitions)
        self.resigns = int((self.reason == MATCH_RESIGN).sum())
        self.aborted = int((self.reason == MATCH_ABORTED).sum())
        self.unfinished = int((self.reason == 0).sum())
        self.scored = int(scored.sum())

        def wdl(mask):
            r = self.result[scored & mask]
            return dict(W=int((r == 1).sum()), D=int((r == 0).sum()), L=int((r == -1).sum()))
        all_ = wdl(np.ones(self.games, bool))
        self.wins, self.draws, self.losses = all_["W"], all_["D"], all_["L"]
        self.by_colour = {"red": wdl(self.a_red == 1), "black": wdl(self.a_red == 0)}
        self.score = (self.wins + 0.5 * self.draws) / self.scored if self.scored else None
        self.elo = elo(self.score)
        self.pentanomial = pentanomial(self.result, self.reason, self.resign is not None, self.tablebase)
        iv = pentanomial_interval(self.pentanomial)
        self.elo_95 = None if iv is None else (elo(iv[1]) if iv[1] > 0 else None, elo(iv[2]) if iv[2] < 1 else None)
        self.simulations = int(simulations)
        self.seconds = float(seconds)
        self.sims_per_s = self.simulations / self.seconds if self.seconds > 0 else 0.0
        self.games_per_s = self.games / self.seconds if self.seconds > 0 else 0.0
        self.players = players

    def to_dict(self):
        """The summary (no per-game arrays): what `python -m cchess_zero_amd.arena` prints.  elo None = infinite (every
        scored game won or lost) or no scored game; an interval end None = unbounded on that side."""
        avoid = dict(avoid_repetition=True, avoided=self.avoided, forced_repetitions=self.forced_repetitions) if self.avoid else {}
        return dict(**avoid, rules=self.rules, mates=self.mates, repetition=self.repetition, repetitions=self.repetitions, perpetuals=self.perpetuals,
                    chase=self.chase, chases=self.chases, resign=self.resign, resigns=self.resigns, tablebase=self.tablebase, tablebases=self.tablebases, games=self.games, scored=self.scored, aborted=self.aborted, unfinished=self.unfinished, W=self.wins,
                    D=self.draws, L=self.losses, by_colour=self.by_colour, score=self.score, elo=self.elo,
                    elo_95=None if self.elo_95 is None else list(self.elo_95), pentanomial=self.pentanomial.tolist(),
                    mean_plies=float(self.plies.mean()) if self.games else 0.0,
                    reasons={REASONS[k]: int((self.reason == k).sum()) for k in REASONS},
                    simulations=self.simulations, seconds=round(self.seconds, 3), sims_per_s=round(self.sims_per_s, 1),
                    games_per_s=round(self.games_per_s, 3), players=self.players)


# ---- ranks ---------------------------------------------------------------------------------------------------------------
def rank_pairs(n_pairs, rank, world):
    """The opening pairs rank `rank` plays: p % world == rank."""
    return np.arange(rank, n_pairs, world)


def merge_ranks(local, n_pairs, rank, world, group=None):
    """Every rank's per-game arrays (local game i = game 2 (rank + world (i // 2)) + i % 2 of the match) -> the whole
    match's arrays on every rank: scattered into zeros and summed with one all_reduce.  local: dict(result, a_red, plies,
    reason, moves [n_local, max_plies] u16 (0xFFFF = none), simulations, seconds); seconds is the slowest rank's."""
    import torch.distributed as dist
    n = 2 * n_pairs
    mp = int(local["moves"].shape[1])
    loc = np.arange(len(local["result"]))
    glob = 2 * (rank + world * (loc // 2)) + loc % 2
    flat = np.zeros((n, 4 + mp), np.int64)
    flat[glob, 0] = local["result"]
    flat[glob, 1] = local["a_red"]
    flat[glob, 2] = local["plies"]
    flat[glob, 3] = local["reason"]
    mv = np.asarray(local["moves"], np.int64)
    flat[glob, 4:] = np.where(mv == 0xFFFF, 0, mv + 1)    # 0 = no move: the sum of one rank's entry and zeros
    backend = dist.get_backend(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    t = torch.from_numpy(flat).to(dev)
    dist.all_reduce(t, group=group)
    s = torch.tensor([float(local["simulations"])], dtype=torch.float64, device=dev)
    dist.all_reduce(s, group=group)
    sec = torch.tensor([float(local["seconds"])], dtype=torch.float64, device=dev)
    dist.all_reduce(sec, op=dist.ReduceOp.MAX, group=group)
    f = t.cpu().numpy()
    moves = np.where(f[:, 4:] == 0, 0xFFFF, f[:, 4:] - 1).astype(np.uint16)
    return dict(result=f[:, 0].astype(np.int8), a_red=f[:, 1].astype(np.uint8), plies=f[:, 2].astype(np.int32),
                reason=f[:, 3].astype(np.uint8), moves=moves, simulations=int(round(float(s.item()))), seconds=float(sec.item()))


# ---- the match -----------------------------------------------------------------------------------------------------------
def _player(p):
    fwd, playouts = p
    if hasattr(fwd, "net") and hasattr(fwd.net, "search_eval"):   # the policy_value_network facade
        fwd = fwd.net
    if hasattr(fwd, "search_eval"):                                # a PolicyValueNet: its device forward, fused path
        fwd = fwd.forward_device
    if not callable(fwd):
        raise TypeError("a player is (PolicyValueNet | policy_value_network | forward(planes) -> (logits, value), playouts)")
    if int(playouts) < 1:
        raise ValueError("a player needs at least one playout per move")
    return fwd, int(playouts)


def _describe(p):
    net = getattr(p[0], "__self__", p[0])
    return dict(playouts=p[1], engine=getattr(net, "engine_name", None) or type(net).__name__,
                blocks=getattr(net, "res_block_nums", None))


class Match:
    """G = slots concurrent games of player A against player B over every opening with both colour assignments.
    max_plies: a game that reaches it is a draw; sample_plies: the first plies of a game are sampled from softmax(log N)
    (temperature 1) with uniforms that are a pure function of (seed, game, ply), the rest are greedy (most visits).
    rules: "capture" — the reference's games: pseudo-legal moves, a game ends when a king is taken; "xiangqi" — the move is
    chosen among the king-safe root children only (cz_movegen_kingsafe), and a mover without one has lost ("mate").
    repetition (rules="xiangqi" only): 0 — no repetition rule; 2..8 — a game ends when its position occurs for that many
    times since the last capture (3 is the usual value): a draw ("repetition"), or a loss for the side that alone checked with
    every move of the cycle ("perpetual") (cz_match_set_repetition).
    chase (with a repetition fold only): False — a chase that repeats is a draw by repetition; True — when neither side checked
    perpetually, a side that alone threatened one and the same unprotected piece after every one of its moves of the cycle has
    lost ("chase"; cz_match_set_chase, Rules.threats).
    resign: None — every game is played out; a value — from ply resign_min_ply of a game on, a mover whose root value (the Q of its
    most visited candidate child, on its own tree) is below it has lost ("resign"; cz_match_set_resign).
    tablebase (rules="xiangqi" only): None — games are played out; a tablebase.Tablebase (all its loaded tables) or a
    tablebase.DeviceSet — a game whose position after a move is in one of the tables ends there with the table's result
    ("tablebase"; cz_match_set_tablebase).  An opening that is itself covered plays one ply first."""

    def __init__(self, player_a, player_b, openings, slots, max_plies=512, sample_plies=0, seed=0, check_every=8,
                 nodes_per_tree=None, rules="capture", repetition=0, chase=False, resign=None, resign_min_ply=0, tablebase=None,
                 avoid_repetition=False):
        check_rule_options("Match", rules, repetition, chase, tablebase, resign_min_ply, avoid=avoid_repetition)
        self.avoid = bool(avoid_repetition)
        self.tablebase = tablebase
        self._tb_own = None
        self.resign = None if resign is None else float(resign)
        self.resign_min_ply = int(resign_min_ply)
        self.rules = rules
        self.repetition = int(repetition)
        self.chase = bool(chase)
        self.players = [_player(player_a), _player(player_b)]
        self.openings = as_openings(openings)
        self.slots = int(slots)
        self.max_plies = int(max_plies)
        self.sample_plies = int(sample_plies)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.check_every = max(1, int(check_every))
        self.nodes_per_tree = nodes_per_tree
        if self.slots < 1 or not 1 <= self.max_plies <= 65535 or self.sample_plies < 0 or len(self.openings) < 1:
            raise ValueError("Match: slots >= 1, 1 <= max_plies <= 65535, sample_plies >= 0 and at least one opening")

    def play(self):
        """Plays every game; -> MatchResult (the same on every rank)."""
        import torch.distributed as dist
        n_pairs = len(self.openings)
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        rank, world = (dist.get_rank(), dist.get_world_size()) if multi else (0, 1)
        mine = rank_pairs(n_pairs, rank, world)
        if len(mine):
            local = self._play_local(self.openings.subset(mine), rank, world)
        else:
            local = dict(result=np.zeros(0, np.int8), a_red=np.zeros(0, np.uint8), plies=np.zeros(0, np.int32),
                         reason=np.zeros(0, np.uint8), moves=np.zeros((0, self.max_plies), np.uint16), simulations=0, seconds=0.0,
                         avoided=(0, 0))
        avoided = local.pop("avoided")
        if multi:
            local = merge_ranks(local, n_pairs, rank, world)
            if self.avoid:
                t = torch.tensor(avoided, dtype=torch.int64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
                dist.all_reduce(t)
                avoided = tuple(int(x) for x in t.tolist())
        return MatchResult(local["result"], local["a_red"], local["plies"], local["reason"], local["moves"], local["simulations"],
                           local["seconds"], [_describe(p) for p in self.players], rules=self.rules, repetition=self.repetition,
                           chase=self.chase, resign=self.resign, tablebase=self.tablebase is not None, avoid=self.avoid, avoided=avoided[0],
                           forced_repetitions=avoided[1])

    def _play_local(self, op, pair_base, pair_stride):
        self.start(op, pair_base, pair_stride)
        try:
            n_games = 2 * len(op)
            limit = (n_games // self.G + 2) * (self.max_plies + 1) + self.check_every
            plies = 0
            torch.cuda.synchronize(self.engines[0].dev)
            t0 = time.perf_counter()
            while True:
                self.step_ply()
                plies += 1
                if plies % self.check_every == 0:
                    fin, _ = self.finished()
                    if fin >= n_games:
                        break
                    if plies > limit:
                        raise RuntimeError("match: %d of %d games finished after %d plies" % (fin, n_games, plies))
            seconds = time.perf_counter() - t0
            out = self.results()
            out["simulations"] = self.finished()[1]
            out["seconds"] = seconds
            out["avoided"] = self.avoid_stats()
            return out
        finally:
            self.close()

    # -- the device loop, one call per stage (play() drives it; tests step it) ----------------------------------------------
    def start(self, op=None, pair_base=0, pair_stride=1):
        """Both engines on G = min(slots, games) slots and the match on the device (cz_match_create): slot g plays game g."""
        op = self.openings if op is None else op
        self.n_games = 2 * len(op)
        G = self.G = min(self.slots, self.n_games)
        dev = torch.device("cuda", torch.cuda.current_device())
        self.engines = []
        for fwd, playouts in self.players:
            pd, ch = plane_format(fwd)
            eng = SearchEngine(G, int(self.nodes_per_tree or pool_nodes(playouts)), dev.index, plane_dtype=pd, channels=ch)
            eng.compact = True   # only the movers' leaves reach each net (fused path)
            eng.reset(np.tile(op.boards[0], (G, 1)), np.zeros(G, np.uint8), None)
            self.engines.append(eng)
        ea, eb = self.engines
        self._op_dev = [torch.from_numpy(x).to(dev) for x in (op.boards, op.side, op.rr)]
        ea.ctx.bind_stream()
        eb.ctx.bind_stream()
        self._h = C.c_void_p()
        call("cz_match_create", ea.ctx.h, eb.ctx.h, *self._op_dev, len(op), int(pair_base), int(pair_stride), self.max_plies, C.byref(self._h))
        set_rule_options("cz_match", self._h, self.rules, self.repetition, self.chase, self.avoid)
        if self.resign is not None:
            call("cz_match_set_resign", self._h, self.resign, self.resign_min_ply)
        if self.tablebase is not None:   # a Tablebase: a set over its loaded tables, this match's to close
            dset, self._tb_own = tablebase_set(self.tablebase)
            call("cz_match_set_tablebase", self._h, dset.h)
        self.masks = [out_pointers("cz_match_active", self._h, 1, player)[0] for player in (0, 1)]
        self.played = torch.empty(G, dtype=torch.int16, device=dev)

    def search(self, player):
        """The playouts of one player over its movers (cz_match_active mask)."""
        fwd, playouts = self.players[player]
        self.engines[player].search(fwd, playouts, active=self.masks[player])

    def choose(self):
        self.engines[0].ctx.bind_stream()
        call("cz_match_choose", self._h, self.sample_plies, C.c_ulonglong(self.seed), self.played)

    def follow(self):
        for eng in self.engines:
            eng.advance(self.played)

    def adjudicate(self):
        self.engines[0].ctx.bind_stream()
        call("cz_match_adjudicate", self._h, self.played)

    def step_ply(self):
        """One ply of every live game: search A over its movers, search B over its movers, choose, advance both, adjudicate."""
        self.search(0)
        self.search(1)
        self.choose()
        self.follow()
        self.adjudicate()

    def finished(self):
        """(games finished, simulations of the searches whose move was chosen) — synchronises."""
        fin, sims = C.c_int32(0), C.c_ulonglong(0)
        call("cz_match_finished", self._h, C.byref(fin), C.byref(sims))
        return int(fin.value), int(sims.value)

    def avoid_stats(self):
        """(plies at which a losing move was taken from the choice, plies at which every move lost) so far — synchronises."""
        a, f = C.c_int32(0), C.c_int32(0)
        call("cz_match_avoid_stats", self._h, C.byref(a), C.byref(f))
        return int(a.value), int(f.value)

    def active(self):
        """(mask of A, mask of B, game of each slot) as host arrays."""
        ptrs = self.masks + [out_pointers("cz_match_results", self._h, 6)[5]]
        return tuple(self.engines[0].ctx.download(p, dt, self.G) for p, dt in zip(ptrs, (np.uint8, np.uint8, np.int32)))

    def history(self):
        """(keys u64 [G, 64], checks u8 [G, 64]) on the host: the slots' position rings (cz_match_history; repetition != 0),
        position i of a slot's game at [i & 63]."""
        return root_rules_history("cz_match", self._h, self.engines[0].ctx, self.G)

    def chase_history(self):
        """chase u64 [G, 64, 4] on the host: the slots' rings of chase records (cz_match_chase_history; chase=True), position i
        of a slot's game at [i & 63] — Rules.threats of that position."""
        return root_rules_chase_history("cz_match", self._h, self.engines[0].ctx, self.G)

    def results(self):
        """The per-game arrays on the host: result, a_red, plies, reason, moves [games, max_plies] (0xFFFF past the end)."""
        n, ptrs = self.n_games, out_pointers("cz_match_results", self._h, 6)
        what = (("result", np.int8, n), ("a_red", np.uint8, n), ("plies", np.int32, n), ("reason", np.uint8, n), ("moves", np.uint16, (n, self.max_plies)))
        return {k: self.engines[0].ctx.download(p, dt, shape) for (k, dt, shape), p in zip(what, ptrs)}

    def close(self):
        if getattr(self, "_h", None):
            lib().cz_match_destroy(self._h)   # gives the table set back
            self._h = None
        if self._tb_own is not None:
            self._tb_own.close()
        self._tb_own = None


# ---- command line --------------------------------------------------------------------------------------------------------
def load_player(path, blocks):
    """A policy_value_network of `blocks` residual blocks with the weights of `path` (own .pt, reference TF bundle, .npz;
    None = fresh weights), default precision."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from policy_value_network import policy_value_network
    # an empty model directory: the net starts from fresh weights, not from whatever ./models holds; the loader's messages
    # stay off the one JSON line
    with contextlib.redirect_stdout(sys.stderr), tempfile.TemporaryDirectory() as empty:
        p = policy_value_network(blocks, save_dir=empty)
        if path:
            p.restore(path)
    return p


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cchess_zero_amd.arena",
                                 description="A match between two checkpoints on the GPU; prints one JSON line.")
    ap.add_argument("--a", default=None, help="checkpoint of player A (own .pt, reference TF bundle, .npz); none = fresh weights")
    ap.add_argument("--b", default=None, help="checkpoint of player B; none = fresh weights")
    ap.add_argument("--blocks", type=int, default=7, help="residual blocks of both nets")
    ap.add_argument("--games", type=int, default=None,
                    help="games (rounded up to an even number: each opening with both colours); default 256, with --all_openings twice their number")
    ap.add_argument("--playout", type=int, default=400, help="playouts per move of A (and of B without --playout_b)")
    ap.add_argument("--playout_b", type=int, default=None, help="playouts per move of B")
    ap.add_argument("--opening_plies", type=int, default=4, help="random plies of the openings")
    ap.add_argument("--all_openings", action="store_true",
                    help="every distinct position after --opening_plies king-safe plies (exhaustive_openings) instead of a random sample")
    ap.add_argument("--book", metavar="B.npz", default=None,
                    help="openings --opening_plies plies into this opening book (book_openings; python -m cchess_zero_amd.book --build) instead of random ones")
    ap.add_argument("--slots", type=int, default=None, help="concurrent games (default: all)")
    ap.add_argument("--seed", type=int, default=0, help="openings and sampled plies")
    ap.add_argument("--max_plies", type=int, default=512, help="a game reaching it is a draw")
    ap.add_argument("--sample_plies", type=int, default=0, help="plies sampled from softmax(log N) at the start of a game")
    add_rule_flags(ap, "the match")
    ap.add_argument("--resign", type=float, default=None,
                    help="a mover whose root value (Q of its most visited move) is below X resigns; default: games are played out")
    ap.add_argument("--resign_min_ply", type=int, default=0, help="with --resign: plies of a game before anybody may resign")
    args = ap.parse_args(argv)
    load_tables = check_rule_flags(ap, args, "arena")
    if args.all_openings and args.book:
        ap.error("--all_openings and --book: one source of openings")
    a = load_player(args.a, args.blocks)
    b = a if args.b == args.a else load_player(args.b, args.blocks)
    if args.all_openings:
        op = exhaustive_openings(args.opening_plies)
        pairs = len(op) if args.games is None else (args.games + 1) // 2
        if pairs > len(op):
            ap.error("--all_openings: %d plies give %d openings, --games %d asks for %d" % (args.opening_plies, len(op), args.games, pairs))
        op = op.subset(np.arange(pairs))
    elif args.book:
        from .book import Book
        pairs = ((256 if args.games is None else args.games) + 1) // 2
        try:
            op = book_openings(Book().load(args.book), pairs, args.opening_plies, args.seed)
        except (OSError, ValueError) as e:
            ap.error("--book: %s" % e)
    else:
        pairs = ((256 if args.games is None else args.games) + 1) // 2
        op = random_openings(pairs, args.opening_plies, args.seed)
    try:
        tb = load_tables()   # under several ranks every rank loads the directory itself
    except ValueError as e:
        ap.error(str(e))
    res = Match((a, args.playout), (b, args.playout_b or args.playout), op, slots=args.slots or 2 * pairs, max_plies=args.max_plies,
                sample_plies=args.sample_plies, seed=args.seed, rules=args.rules, repetition=args.repetition, chase=args.chase, avoid_repetition=args.avoid_repetition,
                resign=args.resign, resign_min_ply=args.resign_min_ply, tablebase=tb).play()
    d = res.to_dict()
    d.update(a=args.a, b=args.b, blocks=args.blocks, opening_plies=args.opening_plies, slots=min(args.slots or 2 * pairs, 2 * pairs),
             seed=args.seed)
    print(json.dumps(d), flush=True)
    return d


if __name__ == "__main__":
    main()
