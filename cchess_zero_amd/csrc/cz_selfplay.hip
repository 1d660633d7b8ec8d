// cz_selfplay.hip — the per-ply bookkeeping of self-play for G concurrent games, device-resident.
//
// Restates, for every game slot of a cz_ctx at once (chengstone/cchess-zero main.py):
//   cchess_main.get_action   :1332-1358   visits -> softmax(log N / T), 0.75 pi + 0.25 Dirichlet(0.3) sampling
//   cchess_main.selfplay     :1493-1554   per-ply (state, pi, mover) lists, game end tests, z assignment, reload
// One wave64 workgroup per game.  Nothing here needs the host: the random numbers come in as device arrays, the
// finished games' records leave through a device ring, finished slots are re-seeded in place, so a loop of
// (search, choose, advance, adjudicate, flush) launches keeps every slot busy for as long as it runs.
//
// Record (CZ_REC_BYTES = 608, include/cchess_hip.h): the root position BEFORE the move, the mover, the root's
// children in generation order with their visit counts, the game result from the mover's point of view.  pi is not
// stored: the reference's pi = softmax(1/T * log(visits)) (main.py:1341) is a pure function of the visit counts, so
// the host recomputes it in float64 with the reference's own expression and gets it bit for bit.
//
// cz_selfplay_set_rules(1) — the games are Xiangqi, as the arena's (cz_match.hip with cz_match_set_rules / _set_repetition): the
// rules act AT THE ROOT ONLY.  The move is chosen, and the record written, over the root children whose move is king-safe; a mover
// without one is mated; with a fold, a fold-th occurrence of the root position ends the game.  The search below the root is
// untouched: in the tree a mate is a king capture two plies down, which it already sees.
//
// cz_selfplay_set_resign — at every rule level a mover whose root value (wave_root_value, cz_internal.h) is below the threshold
// resigns, except in the games drawn to play on, which are played out and counted instead: how often the side that crossed the
// threshold did not lose, and a histogram of the lowest values of the sides that did not lose (CzSpResign, cz_internal.h).
#include "cz_internal.h"

#include <math.h>

namespace {

__global__ __launch_bounds__(64) void k_sp_seed(CzTrees t, CzSelfplay sp, int G, const uint8_t *__restrict__ boards,
                                                const uint8_t *__restrict__ side, const int32_t *__restrict__ rr) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= G) return;
    // the position new games of this slot start from: given, or the tree's current root position
    for (int i = lane; i < CZD_BOARD_LDS; i += 64)
        sp.start_board[(size_t)g * CZD_BOARD_LDS + i] =
            boards ? (i < CZ_NSQ ? boards[(size_t)g * CZ_NSQ + i] : (uint8_t)0) : t.root_board[(size_t)g * CZD_BOARD_LDS + i];
    if (lane == 0) {
        sp.start_side[g] = boards ? (side[g] ? 1 : 0) : t.root_side[g];
        sp.start_rr[g] = boards ? (rr ? rr[g] : 0) : t.root_rr[g];
        sp.ply[g] = 0; sp.stalled[g] = 0; sp.active[g] = 1;
        sp.rr.mated[g] = 0; sp.rr.rep[g] = CZ_REP_NONE;
    }
    if (g == 0)   // every counter starts with the games
        for (int k = lane; k < CZ_SP_NSLOTS; k += 64) sp.stats[k] = 0;
    sp.rr.ring_key[(size_t)g * 64 + lane] = 0ull;
    sp.rr.ring_check[(size_t)g * 64 + lane] = 0;
}

// Resignation's state of slot g for game number game_no of the slot: the play-on draw, no value judged yet, nobody crossed
__device__ __forceinline__ void sp_resign_new_game(const CzSpResign &rs, int g, uint32_t game_no) {
    rs.game_no[g] = game_no;
    rs.playon[g] = sp_plays_on(rs, g, game_no) ? 1 : 0;
    rs.minq[2 * g] = 2.0f; rs.minq[2 * g + 1] = 2.0f;
    rs.would[g] = 0; rs.resigned[g] = 0;
}

// the first cz_selfplay_set_resign after cz_selfplay_begin, on its zeroed block: every slot is in its game 0
__global__ __launch_bounds__(64) void k_sp_resign_init(CzSpResign rs, int G) {
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g < G) sp_resign_new_game(rs, g, 0u);
}

// level >= CZ_RULES_KINGSAFE, before the choice: the root position of every slot, for czk_root_rules_prepare
__global__ __launch_bounds__(64) void k_sp_roots_xq(CzTrees t, CzSelfplay sp, int G) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= G) return;
    wave_gather_root(sp.rr, t, g, sp.active[g] != 0, sp.ply[g], lane);
}

// get_action (main.py:1337-1351) + the record append of selfplay (:1504-1518) for every active game, at rule level LEVEL
// (CzRulesLevel, cz_rootrules.h), over the candidates wave_choose_prologue (cz_rootrules.h) leaves.
// From CZ_RULES_KINGSAFE (cz_selfplay_set_rules(1)) those are the king-safe root children, compacted: pi, the noise (gamma[g][j] of
// compacted child j: a Dirichlet over len(probs) entries), the pick and the record run on them exactly as they run on all n under
// king-capture rules.  None: the mover is mated.  From CZ_RULES_REPETITION the root position's verdict may end the game first.
// On either ending played = 0xFFFF, no record is written and the ply stays; k_sp_adjudicate ends the game.  A forced
// label is played as given.  At every level, with cz_selfplay_set_resign: behind those exits and before the pick the mover's root
// value is judged, and a resignation ends the ply the same way.
template <int LEVEL>
__global__ __launch_bounds__(64) void k_sp_choose(CzTrees t, CzSelfplay sp, int G, const float *__restrict__ gamma,
                                                  const float *__restrict__ u, const uint16_t *__restrict__ forced,
                                                  double inv_temp, float eps, int min_sims, uint16_t *__restrict__ played) {
    constexpr bool XQ = LEVEL >= CZ_RULES_KINGSAFE;
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= G) return;
    if (!sp.active[g]) { if (lane == 0) played[g] = 0xFFFF; return; }
    // asynchronous plies (min_sims > 0): only the games whose search has had its playouts move now — or cannot go on
    // (node pool full: the move is chosen from the visits it has; rules overflow: dropped below)
    if (min_sims > 0 && t.sims[g] < min_sims && (t.status[g] & (CZ_ST_POOL_EXHAUSTED | CZ_ST_NO_MOVES | CZ_ST_MOVE_OVERFLOW)) == 0) {
        if (lane == 0) played[g] = 0xFFFF;
        return;
    }
    if (lane == 0) sp_count(sp, CZ_SP_SIMS, (unsigned long long)t.sims[g]);
    if (XQ && lane == 0) { sp.rr.mated[g] = 0; sp.rr.rep[g] = CZ_REP_NONE; }
    const TreeView v = view_of(t, g);
    const int ply = sp.ply[g];
    int cb, n, N[2], at[2];   // the visits of candidate lane + 64 r and its index among the root's children
    const CzRootFound found = wave_choose_prologue<LEVEL>(sp.rr, t, v, g, ply, lane, cb, n, N, at);
    if (found != CZ_ROOT_CANDIDATES) {
        if (lane == 0) {
            played[g] = 0xFFFF;
            if (found == CZ_ROOT_CANNOT_MOVE) sp.stalled[g] = 1;   // the adjudication drops the game and re-seeds the slot
            if (found == CZ_ROOT_MATED) sp.rr.mated[g] = 1;        // the mover loses
        }
        return;
    }
    uint16_t lab[2] = {0xFFFF, 0xFFFF};
    double pi[2], p[2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (lane + 64 * r < n) lab[r] = v.move[cb + at[r]];
    // cz_selfplay_set_resign: the mover's root value is judged — unless a forced label is played — and a mover below the threshold
    // resigns: played = 0xFFFF, no record, the ply stays, k_sp_adjudicate ends the game.  A play-on game only notes the first crossing.
    if (sp.rs.game_no && sp.rs.threshold == sp.rs.threshold && ply >= sp.rs.min_ply && !(forced && forced[g] < CZ_NLABELS)) {
        float q;
        if (wave_root_value(v, cb, N, at, n, lane, q)) {
            const int mover = t.root_side[g] ? 1 : 0;
            const bool quits = q < sp.rs.threshold && sp.rs.playon[g] == 0;
            if (lane == 0) {
                float *mq = sp.rs.minq + 2 * g + mover;
                if (q < *mq) *mq = q;
                if (q < sp.rs.threshold) {
                    if (quits) { played[g] = 0xFFFF; sp.rs.resigned[g] = 1; }
                    else if (sp.rs.would[g] == 0) sp.rs.would[g] = (uint8_t)(mover + 1);
                }
            }
            if (quits) return;
        }
    }
    if (LEVEL >= CZ_RULES_REPETITION && lane == 0)
        root_count_avoid(sp.rr, g, [&](int k) { sp_count(sp, k ? CZ_SP_FORCED_REPETITIONS : CZ_SP_AVOIDED); });
    wave_visit_policy(N, n, inv_temp, lane, pi);
    double gm[2] = {0.0, 0.0};
    if (gamma && eps > 0.f) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            if (i < n) gm[r] = (double)gamma[(size_t)g * CZD_MAXMOVES + i];
        }
    }
    const double sg = wave_sum(gm[0] + gm[1]);
    const bool noise = gamma && eps > 0.f && sg > 0.0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int i = lane + 64 * r;
        // 0.75 * probs + 0.25 * np.random.dirichlet(0.3 * np.ones(len(probs))), main.py:1346
        p[r] = i < n ? (noise ? (1.0 - (double)eps) * pi[r] + (double)eps * (gm[r] / sg) : pi[r]) : 0.0;
    }
    const int pick = wave_pick_inverse_cdf(p, (double)u[g], lane);
    int mv = __shfl(pick < 64 ? (int)lab[0] : (int)lab[1], pick & 63, 64);
    if (forced && forced[g] < CZ_NLABELS) mv = forced[g];
    // the record of this ply: state before the move, mover, children and their visits
    if (ply < sp.max_plies) {
        uint8_t *rec = sp.hist + ((size_t)g * sp.max_plies + ply) * CZ_REC_BYTES;
        const uint8_t *rb = t.root_board + (size_t)g * CZD_BOARD_LDS;
        for (int i = lane; i < CZ_NSQ; i += 64) rec[i] = rb[i];
        uint16_t *labs = reinterpret_cast<uint16_t *>(rec + CZ_REC_LABELS), *vis = reinterpret_cast<uint16_t *>(rec + CZ_REC_VISITS);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            labs[i] = lab[r];
            vis[i] = (uint16_t)(N[r] > 65535 ? 65535 : N[r]);
        }
        const bool sat = __ballot(N[0] > 65535 || N[1] > 65535) != 0ull;
        if (lane == 0) {
            rec[CZ_REC_SIDE] = t.root_side[g];
            rec[CZ_REC_COUNT] = (uint8_t)n;
            rec[CZ_REC_Z] = 0;
            rec[CZ_REC_FLAGS] = sat ? 1 : 0;   // bit 0: a visit count saturated the 16-bit field
            *reinterpret_cast<uint16_t *>(rec + CZ_REC_PLY) = (uint16_t)ply;
        }
    }
    if (lane == 0) { played[g] = (uint16_t)mv; sp.ply[g] = ply + 1; }
}

// The game-end tests of selfplay (main.py:1532-1545) on the position after the move, z for every recorded ply, and —
// reseed != 0 — MCTS_tree.reload / GameBoard.reload for the next game of the slot (:1549-1551, :1494).
// fin_n[g] = number of records the finished game hands to the ring (0: not finished, or dropped).
// Whether and how the game ended is wave_game_end's answer (cz_internal.h: the one precedence of the endings); `aborted` here is a
// stalled choose or a played label that is no root child, and such a game is dropped with no record.  From CZ_RULES_KINGSAFE the
// endings the last choose found on the root it left untouched come first — a repetition verdict (a draw, or a loss for the side
// that checked perpetually), then a mated mover (the side to move loses); z as for a king capture.  At CZ_RULES_CHASE the verdict
// may be a chase — a loss for the side that chased, z as for perpetual check, counted in CZ_SP_CHASES and not among the perpetuals.
// cz_selfplay_set_resign, at every level: a game the last choose resigned is lost by the side to move, z as for a king capture;
// a play-on game that ends here — however it ends, unless it stalled — goes into the play-on counters and the histogram; the
// slot's resignation state starts over with its next game.
// cz_selfplay_set_tablebase: sp.tb_value[g] is what the attached set answers for the position after the move (k_tb_probe_set, the
// launch in front of this one; CZ_TB_MISS for a slot whose `played` is no label); a covered value ends the game at its place in
// wave_game_end's precedence, z and the counters as for a king capture, and CZ_SP_TABLEBASE counts it.
template <int LEVEL>
__global__ __launch_bounds__(64) void k_sp_adjudicate(CzTrees t, CzSelfplay sp, int G, int reseed, const uint16_t *__restrict__ played,
                                                      int32_t *__restrict__ fin_n) {
    constexpr bool XQ = LEVEL >= CZ_RULES_KINGSAFE;
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= G) return;
    if (!sp.active[g]) { if (lane == 0) fin_n[g] = 0; return; }
    // cz_selfplay_set_resign: the last choose resigned the game
    const bool resigned = sp.rs.game_no && sp.rs.resigned[g] != 0;
    // asynchronous plies: only the slots that just moved (or stalled, or ended by the rules or by resignation) can have ended their game
    if (played && played[g] == 0xFFFF && !sp.stalled[g] && !resigned && !(XQ && (sp.rr.rep[g] != CZ_REP_NONE || sp.rr.mated[g] != 0))) {
        if (lane == 0) fin_n[g] = 0;
        return;
    }
    const int ply = sp.ply[g];
    const bool aborted = sp.stalled[g] != 0 || (t.status[g] & CZ_ST_BAD_ADVANCE) != 0;
    const int tb = sp.tb_value ? (int)sp.tb_value[g] : CZ_TB_MISS;
    const CzGameEnd end = wave_game_end<LEVEL>(sp.rr, g, resigned, aborted, tb, t.root_board + (size_t)g * CZD_BOARD_LDS, t.root_rr[g], t.root_side[g], ply,
                                               sp.max_plies, lane);
    if (!end.how) { if (lane == 0) fin_n[g] = 0; return; }
    const bool stalled = end.how == CZ_MATCH_ABORTED, decided = end.loser >= 0;   // neither: a draw
    const int winner = 1 - end.loser;
    const int n = stalled ? 0 : min(ply, sp.max_plies);
    for (int j = lane; j < n; j += 64) {
        uint8_t *rec = sp.hist + ((size_t)g * sp.max_plies + j) * CZ_REC_BYTES;
        // z[current_players == winner] = 1, else -1 (main.py:1538-1539); zeros for a tie (:1543)
        const int z = decided ? (rec[CZ_REC_SIDE] == winner ? 1 : -1) : 0;
        rec[CZ_REC_Z] = (uint8_t)(int8_t)z;
    }
    if (lane == 0) {
        fin_n[g] = n;
        sp_count(sp, CZ_SP_GAMES);
        sp_count(sp, stalled ? CZ_SP_STALLED : decided ? (winner ? CZ_SP_BLACK_WINS : CZ_SP_RED_WINS) : CZ_SP_DRAWS);
        sp_count(sp, CZ_SP_PLIES, (unsigned long long)n);
        if (end.how == CZ_MATCH_TABLEBASE) sp_count(sp, CZ_SP_TABLEBASE);
        if constexpr (XQ) {
            if (end.how == CZ_MATCH_CHASE) sp_count(sp, CZ_SP_CHASES);
            else if (end.how == CZ_MATCH_MATE) sp_count(sp, CZ_SP_MATES);
            else if (end.how == CZ_MATCH_REPETITION || end.how == CZ_MATCH_PERPETUAL) sp_count(sp, end.how == CZ_MATCH_REPETITION ? CZ_SP_REPETITIONS : CZ_SP_PERPETUALS);
            sp.rr.mated[g] = 0; sp.rr.rep[g] = CZ_REP_NONE;
        }
        if (sp.rs.game_no) {
            if (end.how == CZ_MATCH_RESIGN) sp_count(sp, CZ_SP_RESIGNED);
            if (sp.rs.playon[g] && !stalled) {   // what the game would have done had it not played on, against how it ended
                const int loser = end.loser, would = sp.rs.would[g];
                sp_count(sp, CZ_SP_PLAYON_GAMES);
                if (would) {
                    sp_count(sp, CZ_SP_PLAYON_WOULD);
                    if (loser != would - 1) sp_count(sp, CZ_SP_PLAYON_FALSE);   // the side that would have resigned won or drew
                }
                for (int s = 0; s < 2; ++s) {
                    const float q = sp.rs.minq[2 * g + s];
                    if (loser != s && q < 2.0f) sp_count(sp, CZ_SP_RESIGN_HIST + min(max((int)floorf((q + 1.0f) * 32.0f), 0), 63));
                }
            }
            // the slot's next game (reseed), or a parked slot with nothing left over
            sp_resign_new_game(sp.rs, g, sp.rs.game_no[g] + (reseed ? 1u : 0u));
        }
    }
    if (reseed) {   // the slot's next game: a fresh root on its start position
        fresh_root(t, g, lane, sp.start_board, CZD_BOARD_LDS, sp.start_side, sp.start_rr, g);
        if (lane == 0) { sp.ply[g] = 0; sp.stalled[g] = 0; }
    } else if (lane == 0) sp.active[g] = 0;
}
// Copies the records of the games k_sp_adjudicate finished to ring[(offset[g] + j) % ring_records].  The offsets are an
// exclusive prefix sum of fin_n computed by the caller (record order = game order: deterministic, no atomics).
__global__ __launch_bounds__(64) void k_sp_flush(CzSelfplay sp, int G, const int32_t *__restrict__ fin_n,
                                                 const long long *__restrict__ offset, uint8_t *__restrict__ ring,
                                                 long long ring_records, const long long *__restrict__ read_cursor) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= G) return;
    const int n = fin_n[g];
    if (n <= 0) return;
    const long long off = offset[g];
    if (read_cursor && off + n - *read_cursor > ring_records) {   // would overwrite records nobody has read yet
        if (lane == 0) sp_count(sp, CZ_SP_DROPPED, (unsigned long long)n);
        return;
    }
    for (int j = 0; j < n; ++j) {
        const uint4 *src = reinterpret_cast<const uint4 *>(sp.hist + ((size_t)g * sp.max_plies + j) * CZ_REC_BYTES);
        uint4 *dst = reinterpret_cast<uint4 *>(ring + (size_t)((off + j) % ring_records) * CZ_REC_BYTES);
        if (lane < CZ_REC_BYTES / 16) dst[lane] = src[lane];
    }
}

}  // namespace

// ---- the entry points, in cz_match.hip's order: create, setters, getters, choose, adjudicate ------------------------
// The state lives in cz_ctx: sp in sp_block, sp.rs in sp_resign_block, and sp_root (CzRootHost, cz_internal.h) with the chase
// part of sp.rr and sp.tb_value in its own two blocks.  cz_destroy frees all four.

int cz_selfplay_begin(cz_ctx *c, int max_plies, const uint8_t *boards, const uint8_t *side, const int32_t *rr) {
    CZ_REQUIRE(c && c->G > 0, "cz_selfplay_begin: call cz_search_reset first");
    CZ_REQUIRE(max_plies >= 1 && max_plies <= 65535, "cz_selfplay_begin: 1 <= max_plies <= 65535");
    CZ_REQUIRE(boards == nullptr || side != nullptr, "cz_selfplay_begin: start_side required with start_boards");
    if (!c->sp_block || c->sp.max_plies != max_plies) {
        CZ_HIP(hipStreamSynchronize(c->stream));
        if (c->sp_block) { (void)hipFree(c->sp_block); c->sp_block = nullptr; }
        const size_t G = (size_t)c->max_games;
        CzSelfplay &sp = c->sp;
        const int rc = carve_alloc(&c->sp_block, c->stream, false, "cz_selfplay_begin", [&](Carver &k) {
            sp.hist = k.take<uint8_t>(G * (size_t)max_plies * CZ_REC_BYTES);
            sp.ply = k.take<int32_t>(G);
            sp.stalled = k.take<uint8_t>(G);
            sp.active = k.take<uint8_t>(G);
            sp.start_board = k.take<uint8_t>(G * CZD_BOARD_LDS);
            sp.start_side = k.take<uint8_t>(G);
            sp.start_rr = k.take<int32_t>(G);
            sp.stats = k.take<long long>(CZ_SP_NSLOTS);
            carve_root_rules(k, sp.rr, G, false);
        });
        if (rc != CZ_OK) return rc;
        sp.max_plies = max_plies;
    }
    // rules, fold and chase off, no table set (it needs rules 1).  Nothing may change after the first choose; sp.rr's arrays
    // other than the chase part are sp_block's; the chase rings are cleared whenever the rule is switched on
    cz_root_begin(c->sp_root, CzRootHost{"cz_selfplay", "ctx", "the history starts at the games' first positions", false, false, true, c,
                                         c->max_games, &c->sp.rr, &c->sp.tb_value});
    c->sp.rs = CzSpResign{};   // resignation off: no pointer, no kernel looks
    c->sp.rs.threshold = NAN;
    hipLaunchKernelGGL(k_sp_seed, dim3(c->G), dim3(64), 0, c->stream, c->t, c->sp, c->G, boards, side, rr);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_selfplay_set_rules(cz_ctx *c, int rules) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_set_rules: call cz_selfplay_begin first");
    return cz_root_set_rules(c->sp_root, rules);
}

int cz_selfplay_set_repetition(cz_ctx *c, int fold) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_set_repetition: call cz_selfplay_begin first");
    return cz_root_set_repetition(c->sp_root, fold);
}

int cz_selfplay_history(cz_ctx *c, const uint64_t **keys, const uint8_t **checks) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_history: cz_selfplay_set_repetition first");
    return cz_root_history(c->sp_root, keys, checks);
}

int cz_selfplay_set_chase(cz_ctx *c, int on) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_set_chase: call cz_selfplay_begin first");
    return cz_root_set_chase(c->sp_root, on);
}

int cz_selfplay_chase_history(cz_ctx *c, const uint64_t **chase) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_chase_history: cz_selfplay_set_chase first");
    return cz_root_chase_history(c->sp_root, chase);
}

int cz_selfplay_set_avoid(cz_ctx *c, int on) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_set_avoid: call cz_selfplay_begin first");
    return cz_root_set_avoid(c->sp_root, on);
}

int cz_selfplay_set_resign(cz_ctx *c, float threshold, int min_ply, double playon_fraction, unsigned long long seed) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_set_resign: call cz_selfplay_begin first");
    CZ_REQUIRE(min_ply >= 0 && playon_fraction >= 0.0 && playon_fraction <= 1.0, "cz_selfplay_set_resign: min_ply >= 0 and 0 <= playon_fraction <= 1 required");
    CzSpResign &rs = c->sp.rs;
    if (rs.game_no) {   // a later call retunes: the per-game state, the counters and the seed stay
        rs.threshold = threshold; rs.min_ply = min_ply; rs.playon_fraction = playon_fraction;
        return CZ_OK;
    }
    if (threshold != threshold) return CZ_OK;   // off stays off
    const size_t G = (size_t)c->max_games;
    CzSpResign r{};   // c->sp.rs stays "off" until the block stands
    r.threshold = threshold; r.min_ply = min_ply; r.playon_fraction = playon_fraction; r.seed = seed;
    const int rc = carve_alloc(&c->sp_resign_block, c->stream, true, "cz_selfplay_set_resign", [&](Carver &k) {
        r.game_no = k.take<uint32_t>(G);
        r.playon = k.take<uint8_t>(G);
        r.minq = k.take<float>(G * 2);
        r.would = k.take<uint8_t>(G);
        r.resigned = k.take<uint8_t>(G);
    });
    if (rc != CZ_OK) return rc;
    rs = r;
    hipLaunchKernelGGL(k_sp_resign_init, dim3((c->max_games + 63) / 64), dim3(64), 0, c->stream, c->sp.rs, c->max_games);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_selfplay_set_tablebase(cz_ctx *c, cz_tb_set *set) {
    CZ_REQUIRE(c && c->sp_block, "cz_selfplay_set_tablebase: call cz_selfplay_begin first");
    return cz_root_set_tablebase(c->sp_root, set);
}

int cz_selfplay_active(cz_ctx *c, const uint8_t **active) {
    CZ_REQUIRE(c && c->sp_block && active, "cz_selfplay_active: call cz_selfplay_begin first");
    *active = c->sp.active;
    return CZ_OK;
}

int cz_selfplay_choose(cz_ctx *c, const float *gamma, const float *u, const uint16_t *forced, double temperature, float eps, int min_sims, uint16_t *played) {
    CZ_REQUIRE(c && c->sp_block && c->G > 0, "cz_selfplay_choose: call cz_selfplay_begin first");
    CZ_REQUIRE(u && played, "cz_selfplay_choose: u and played required");
    CZ_REQUIRE(temperature > 0.0 && eps >= 0.f && eps <= 1.f, "cz_selfplay_choose: temperature > 0 and 0 <= noise_eps <= 1 required");
    CZ_REQUIRE(min_sims >= 0, "cz_selfplay_choose: min_sims >= 0 required");
    return cz_root_choose(
        c->sp_root, c->G, [&] { hipLaunchKernelGGL(k_sp_roots_xq, dim3(c->G), dim3(64), 0, c->stream, c->t, c->sp, c->G); },
        [&](auto L) {
            hipLaunchKernelGGL(k_sp_choose<decltype(L)::value>, dim3(c->G), dim3(64), 0, c->stream, c->t, c->sp, c->G, gamma, u, forced, 1.0 / temperature,
                               eps, min_sims, played);
        });
}

int cz_selfplay_adjudicate(cz_ctx *c, int reseed, const uint16_t *played, int32_t *fin_n) {
    CZ_REQUIRE(c && c->sp_block && c->G > 0 && fin_n, "cz_selfplay_adjudicate: call cz_selfplay_begin first / null fin_n");
    return cz_root_adjudicate(c->sp_root, played, c->G, [&](auto L) {
        hipLaunchKernelGGL(k_sp_adjudicate<decltype(L)::value>, dim3(c->G), dim3(64), 0, c->stream, c->t, c->sp, c->G, reseed, played, fin_n);
    });
}

int cz_selfplay_flush(cz_ctx *c, const int32_t *fin_n, const long long *offset, uint8_t *ring, long long ring_records, const long long *read_cursor) {
    CZ_REQUIRE(c && c->sp_block && c->G > 0, "cz_selfplay_flush: call cz_selfplay_begin first");
    CZ_REQUIRE(fin_n && offset && ring && ring_records > 0, "cz_selfplay_flush: null argument / empty ring");
    hipLaunchKernelGGL(k_sp_flush, dim3(c->G), dim3(64), 0, c->stream, c->sp, c->G, fin_n, offset, ring, ring_records, read_cursor);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

// The five getters: slots first .. first + n - 1 of sp.stats (CzSpSlot), device to device.  A rule that is off reads the zeros
// cz_selfplay_begin left: its slots are counted only while it is on, and it is switched on after a begin.
static int sp_stats_slice(cz_ctx *c, const char *who, long long *dst, int first, int n) {
    if (!(c && c->sp_block && dst)) { cz_set_error("%s: call cz_selfplay_begin first / null argument", who); return CZ_EINVAL; }
    CZ_HIP(hipMemcpyAsync(dst, c->sp.stats + first, sizeof(long long) * n, hipMemcpyDeviceToDevice, c->stream));
    return CZ_OK;
}
int cz_selfplay_stats(cz_ctx *c, long long *stats_dev) { return sp_stats_slice(c, "cz_selfplay_stats", stats_dev, 0, CZ_SP_NSTATS); }
int cz_selfplay_rules_stats(cz_ctx *c, long long *stats_dev) { return sp_stats_slice(c, "cz_selfplay_rules_stats", stats_dev, CZ_SP_MATES, 3); }
int cz_selfplay_chase_stats(cz_ctx *c, long long *stats_dev) { return sp_stats_slice(c, "cz_selfplay_chase_stats", stats_dev, CZ_SP_CHASES, 1); }
int cz_selfplay_tablebase_stats(cz_ctx *c, long long *stats_dev) { return sp_stats_slice(c, "cz_selfplay_tablebase_stats", stats_dev, CZ_SP_TABLEBASE, 1); }
int cz_selfplay_avoid_stats(cz_ctx *c, long long *stats_dev) { return sp_stats_slice(c, "cz_selfplay_avoid_stats", stats_dev, CZ_SP_AVOIDED, 2); }
int cz_selfplay_resign_stats(cz_ctx *c, long long *stats_dev, long long *hist_dev) {
    if (const int rc = sp_stats_slice(c, "cz_selfplay_resign_stats", stats_dev, CZ_SP_RESIGNED, 4)) return rc;
    return hist_dev ? sp_stats_slice(c, "cz_selfplay_resign_stats", hist_dev, CZ_SP_RESIGN_HIST, 64) : CZ_OK;
}
