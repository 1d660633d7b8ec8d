// cz_match.hip — the per-ply bookkeeping of an evaluation match between two players, device-resident.
//
// Restates, for G concurrent games at once (chengstone/cchess-zero main.py):
//   cchess_main.policy_evaluate  :1207-1222   a match of the current net against an opponent (commented out there)
//   cchess_main.get_action       :1332-1341   the move: the most visited root child (T -> 0), or softmax(log N) at T = 1
//   cchess_main.human_move       :272-276     the opponent's tree follows the move played (update_tree)
//   cchess_main.check_end        :1380-1392   a king is gone, or 60 plies without a capture
// Each player has its own cz_ctx (its own trees, net and playout budget); slot g of both contexts belongs to the same game.
// One wave64 workgroup per slot.  Games come from a queue: game i plays opening i / 2 with player A red when i is even,
// so every opening is played once with each colour assignment.  A slot whose game ends takes the next game of the queue
// at once, or parks when the queue is empty.  The host only reads the finished-games counter every few plies.
#include "cz_internal.h"

// The device view of a match: per slot the game it plays, per game the result.
struct CzMatch {
    int G, n_games, max_plies;
    long long pair_base, pair_stride;
    const uint8_t *open_board;    // [n_games / 2][90]
    const uint8_t *open_side;     // [n_games / 2]
    const int32_t *open_rr;       // [n_games / 2]
    int32_t *queue;               // [4] next game to hand out, games finished; cz_match_set_avoid: plies with a move removed, plies at which every move loses
    unsigned long long *sims;     // [1] simulations of the searches whose move was chosen
    int32_t *game;                // [G] game of the slot, -1 = parked
    int32_t *ply;                 // [G] plies played in the slot's game
    uint8_t *mover_a;             // [G] player A is to move in the slot's game
    uint8_t *act_a, *act_b;       // [G] mover masks: this player is to move and the game is live
    uint8_t *stalled;             // [G] the last choose found no root child
    uint8_t *resigned;            // [G] the last choose found the mover's root value below resign_threshold
    float resign_threshold;       // cz_match_set_resign; NaN: nobody resigns
    int resign_min_ply;
    int8_t *result;              // [n_games] +1 / 0 / -1 from A's point of view
    uint8_t *a_red;               // [n_games] 1: A played red
    int32_t *plies;               // [n_games]
    uint8_t *reason;              // [n_games] CZ_MATCH_*
    uint16_t *moves;              // [n_games][max_plies] labels played, 0xFFFF past the end
    CzRootRules rr;               // rules = 1: the rules at the root (cz_rootrules.h), of the mover's root positions; NULL before
    int16_t *tb_value;            // [G] cz_match_set_tablebase: the set's value of the slot's position after the move; NULL while off
};

struct cz_match {
    cz_ctx *a, *b;
    int G, n_games;
    CzMatch m;                          // the arrays inside block; m.rr and m.tb_value inside root's blocks
    void *block;
    CzRootHost root;                    // the rules at the root and the table set (cz_internal.h), over m.rr and m.tb_value
};

namespace {

// the uniform of a sampled move (include/cchess_hip.h cz_match_choose): a pure function of (seed, global game, ply)
__device__ __forceinline__ double match_uniform(unsigned long long seed, long long game, int ply) {
    return uniform53(splitmix64(seed ^ splitmix64(((unsigned long long)game << 16) | (unsigned long long)ply)));
}

__device__ __forceinline__ long long global_game(const CzMatch &m, int game) {
    return 2 * (m.pair_base + m.pair_stride * (long long)(game >> 1)) + (game & 1);
}

// slot g takes game `game` of the queue (both trees on its opening), or parks (game >= n_games): both trees keep a
// fresh root with no simulation, and neither mover mask names the slot, so no search touches it again
__device__ __forceinline__ void take_game(const CzTrees &ta, const CzTrees &tb, const CzMatch &m, int g, int game, int lane) {
    if (game < m.n_games) {
        const int p = game >> 1;
        fresh_root(ta, g, lane, m.open_board, CZ_NSQ, m.open_side, m.open_rr, p);
        fresh_root(tb, g, lane, m.open_board, CZ_NSQ, m.open_side, m.open_rr, p);
        if (lane == 0) {
            const bool a_red = (game & 1) == 0;
            const bool ma = (m.open_side[p] == 0) == a_red;
            m.game[g] = game; m.ply[g] = 0; m.stalled[g] = 0;
            m.mover_a[g] = ma ? 1 : 0; m.act_a[g] = ma ? 1 : 0; m.act_b[g] = ma ? 0 : 1;
        }
    } else {
        fresh_root(ta, g, lane);
        fresh_root(tb, g, lane);
        if (lane == 0) { m.game[g] = -1; m.act_a[g] = 0; m.act_b[g] = 0; m.stalled[g] = 0; }
    }
}

__global__ __launch_bounds__(64) void k_match_start(CzTrees ta, CzTrees tb, CzMatch m) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    if (g == 0 && lane == 0) { m.queue[0] = min(m.G, m.n_games); m.queue[1] = 0; m.queue[2] = 0; m.queue[3] = 0; *m.sims = 0ull; }
    take_game(ta, tb, m, g, g, lane);
}

// get_action of the mover (main.py:1332-1341) on its own tree, at rule level LEVEL (CzRulesLevel, cz_rootrules.h): greedy, or
// sampled for the game's first sample_plies plies (select_move -> get_action(state, temperature = 1), main.py:1123,1433-1435: no
// Dirichlet noise), among the candidates wave_choose_prologue (cz_rootrules.h) leaves.  On each of its endings no move is logged
// and the ply stays (k_match_adjudicate).
// At every level, with cz_match_set_resign: behind those exits and before the choice, a mover whose root value (wave_root_value,
// cz_internal.h) is below the threshold resigns — the game ends the same way, as CZ_MATCH_RESIGN.
template <int LEVEL>
__global__ __launch_bounds__(64) void k_match_choose(CzTrees ta, CzTrees tb, CzMatch m, int sample_plies, unsigned long long seed,
                                                     uint16_t *__restrict__ played) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) { if (lane == 0) played[g] = 0xFFFF; return; }   // a parked slot: before any ring is touched
    const CzTrees &t = m.mover_a[g] ? ta : tb;
    if (lane == 0) atomicAdd(m.sims, (unsigned long long)t.sims[g]);
    if (LEVEL >= CZ_RULES_KINGSAFE && lane == 0) m.rr.mated[g] = 0;   // rr.rep is cleared when a game ends (k_match_adjudicate)
    const TreeView v = view_of(t, g);
    const int ply = m.ply[g];
    int cb, n, N[2], at[2];
    const CzRootFound found = wave_choose_prologue<LEVEL>(m.rr, t, v, g, ply, lane, cb, n, N, at);
    if (found != CZ_ROOT_CANDIDATES) {
        if (lane == 0) {
            played[g] = 0xFFFF;
            if (found == CZ_ROOT_CANNOT_MOVE) m.stalled[g] = 1;   // the game is aborted by the adjudication
            if (found == CZ_ROOT_MATED) m.rr.mated[g] = 1;        // the mover loses
        }
        return;
    }
    if (m.resign_threshold == m.resign_threshold) {   // cz_match_set_resign: the mover resigns on its own tree's value, sampled plies too
        float q;
        if (ply >= m.resign_min_ply && wave_root_value(v, cb, N, at, n, lane, q) && q < m.resign_threshold) {
            if (lane == 0) { played[g] = 0xFFFF; m.resigned[g] = 1; }   // no move is logged, the ply stays (k_match_adjudicate)
            return;
        }
    }
    if (LEVEL >= CZ_RULES_REPETITION && lane == 0) root_count_avoid(m.rr, g, [&](int k) { atomicAdd(&m.queue[2 + k], 1); });
    int pick;
    if (ply < sample_plies) {
        double pi[2];
        wave_visit_policy(N, n, 1.0, lane, pi);
        pick = wave_pick_inverse_cdf(pi, match_uniform(seed, global_game(m, game), ply), lane);
    } else {
        pick = wave_most_visited(N, n, lane);
    }
    pick = __shfl(pick < 64 ? at[0] : at[1], pick & 63, 64);
    if (lane == 0) {
        const uint16_t mv = v.move[cb + pick];
        if (ply < m.max_plies) m.moves[(size_t)game * m.max_plies + ply] = mv;
        played[g] = mv;
        m.ply[g] = ply + 1;
    }
}

// level >= CZ_RULES_KINGSAFE, before the choice: the mover's root position of every slot, for czk_root_rules_prepare
__global__ __launch_bounds__(64) void k_match_roots_xq(CzTrees ta, CzTrees tb, CzMatch m) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    wave_gather_root(m.rr, m.mover_a[g] ? ta : tb, g, m.game[g] >= 0, m.ply[g], lane);
}

// After cz_search_advance(played) on both contexts: the follower's failed advance (its root was never expanded, so it has no
// child for the move) is its normal case — it starts a fresh root on the new position; then check_end (main.py:1380-1392)
// plus the match's own endings (ply cap, aborted game), the result, and the slot's next game.  Whether and how the game ended
// is wave_game_end's answer (cz_internal.h: the one precedence of the endings, in the match's own CZ_MATCH_* codes), the result
// follows from the side it names as the loser; `aborted` here is a stalled choose, no label played, or a label that is no child
// of the mover's root.  cz_match_set_tablebase: m.tb_value[g] is the attached set's value of the position after the move
// (k_tb_probe_set, the launch in front of this one; CZ_TB_MISS for a slot whose `played` is no label).
template <int LEVEL>
__global__ __launch_bounds__(64) void k_match_adjudicate(CzTrees ta, CzTrees tb, CzMatch m, const uint16_t *__restrict__ played) {
    constexpr bool XQ = LEVEL >= CZ_RULES_KINGSAFE, REP = LEVEL >= CZ_RULES_REPETITION;
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) return;
    const bool ma = m.mover_a[g] != 0;
    const CzTrees &mv = ma ? ta : tb, &fo = ma ? tb : ta;   // the mover's tree, the follower's
    const bool aborted = m.stalled[g] != 0 || played[g] >= CZ_NLABELS || (mv.status[g] & CZ_ST_BAD_ADVANCE) != 0;
    const int ply = m.ply[g];
    const int tbv = m.tb_value ? (int)m.tb_value[g] : CZ_TB_MISS;
    const CzGameEnd end = wave_game_end<LEVEL>(m.rr, g, m.resigned[g] != 0, aborted, tbv, mv.root_board + (size_t)g * CZD_BOARD_LDS, mv.root_rr[g],
                                               mv.root_side[g], ply, m.max_plies, lane);
    if (lane == 0) fo.status[g] &= ~CZ_ST_BAD_ADVANCE;
    if (!end.how) {
        if (lane == 0) { m.mover_a[g] = ma ? 0 : 1; m.act_a[g] = ma ? 0 : 1; m.act_b[g] = ma ? 1 : 0; }
        return;
    }
    int next = 0;
    if (lane == 0) {
        const bool a_red = (game & 1) == 0;
        const int8_t result = (int8_t)(end.loser < 0 ? 0 : ((end.loser == 0) == a_red ? -1 : 1));   // -1: A has the losing colour
        m.result[game] = result;
        if (XQ) m.rr.mated[g] = 0;
        if constexpr (REP) m.rr.rep[g] = CZ_REP_NONE;
        m.resigned[g] = 0;
        m.a_red[game] = a_red ? 1 : 0;
        m.plies[game] = ply;
        m.reason[game] = (uint8_t)end.how;
        atomicAdd(&m.queue[1], 1);
        next = atomicAdd(&m.queue[0], 1);
    }
    next = __shfl(next, 0, 64);
    take_game(ta, tb, m, g, next, lane);
}

}  // namespace

// the match's arrays inside its one allocation
static void carve(Carver &k, CzMatch &m, size_t G, size_t n) {
    const size_t np = n / 2;
    m.open_board = k.take<uint8_t>(np * CZ_NSQ);
    m.open_side = k.take<uint8_t>(np);
    m.open_rr = k.take<int32_t>(np);
    m.queue = k.take<int32_t>(4);
    m.sims = k.take<unsigned long long>(1);
    m.game = k.take<int32_t>(G);
    m.ply = k.take<int32_t>(G);
    m.mover_a = k.take<uint8_t>(G);
    m.act_a = k.take<uint8_t>(G);
    m.act_b = k.take<uint8_t>(G);
    m.stalled = k.take<uint8_t>(G);
    m.resigned = k.take<uint8_t>(G);
    m.result = k.take<int8_t>(n);
    m.a_red = k.take<uint8_t>(n);
    m.plies = k.take<int32_t>(n);
    m.reason = k.take<uint8_t>(n);
    m.moves = k.take<uint16_t>(n * (size_t)m.max_plies);
}

int cz_match_create(cz_ctx *a, cz_ctx *b, const uint8_t *boards, const uint8_t *side, const int32_t *rr, int n_openings,
                    long long pair_base, long long pair_stride, int max_plies, cz_match **out) {
    CZ_REQUIRE(out, "cz_match_create: null out");
    *out = nullptr;
    CZ_REQUIRE(a && b && a != b, "cz_match_create: two distinct contexts required");
    CZ_REQUIRE(a->G > 0 && a->G == b->G, "cz_match_create: cz_search_reset both contexts to the same number of slots first");
    CZ_REQUIRE(a->device == b->device && a->stream == b->stream, "cz_match_create: both contexts must be bound to the same device and stream");
    CZ_REQUIRE(a->width == 1 && b->width == 1, "cz_match_create: players search with width 1");
    CZ_REQUIRE(boards && side && n_openings >= 1 && n_openings <= (1 << 29), "cz_match_create: 1 <= n_openings and opening arrays required");
    CZ_REQUIRE(pair_base >= 0 && pair_stride >= 1, "cz_match_create: pair_base >= 0, pair_stride >= 1");
    CZ_REQUIRE(max_plies >= 1 && max_plies <= 65535, "cz_match_create: 1 <= max_plies <= 65535");
    cz_match *mh = new cz_match();
    mh->a = a; mh->b = b; mh->G = a->G; mh->n_games = 2 * n_openings;
    CzMatch &m = mh->m;
    m.G = mh->G; m.n_games = mh->n_games; m.max_plies = max_plies; m.pair_base = pair_base; m.pair_stride = pair_stride;
    m.resign_threshold = NAN; m.resign_min_ply = 0;
    // the rules may change between two plies; m.rr's arrays are all the root's own, zeroed once when they are made
    cz_root_begin(mh->root, CzRootHost{"cz_match", "match", "the history starts at the openings", true, true, false, a, mh->G, &m.rr, &m.tb_value});
    const size_t np = (size_t)n_openings;
    int rc = carve_alloc(&mh->block, a->stream, true, "cz_match_create", [&](Carver &k) { carve(k, m, (size_t)mh->G, (size_t)mh->n_games); });
    auto fail = [&](hipError_t e, const char *what) {
        cz_set_error("cz_match_create: %s failed: %s", what, hipGetErrorString(e));
        rc = CZ_EHIP;
    };
    hipError_t e;
    if (rc == CZ_OK) {
        if ((e = hipMemsetAsync(m.moves, 0xFF, (size_t)mh->n_games * max_plies * 2, a->stream)) != hipSuccess) fail(e, "hipMemsetAsync");
        else if ((e = hipMemcpyAsync((void *)m.open_board, boards, np * CZ_NSQ, hipMemcpyDeviceToDevice, a->stream)) != hipSuccess) fail(e, "hipMemcpyAsync");
        else if ((e = hipMemcpyAsync((void *)m.open_side, side, np, hipMemcpyDeviceToDevice, a->stream)) != hipSuccess) fail(e, "hipMemcpyAsync");
        else if (rr && (e = hipMemcpyAsync((void *)m.open_rr, rr, np * 4, hipMemcpyDeviceToDevice, a->stream)) != hipSuccess) fail(e, "hipMemcpyAsync");
    }
    if (rc == CZ_OK) {
        hipLaunchKernelGGL(k_match_start, dim3(mh->G), dim3(64), 0, a->stream, a->t, b->t, m);
        if ((e = hipGetLastError()) != hipSuccess) fail(e, "k_match_start");
    }
    if (rc != CZ_OK) {
        (void)hipStreamSynchronize(a->stream);
        (void)hipFree(mh->block);
        delete mh;
        return rc;
    }
    *out = mh;
    return CZ_OK;
}

// a setter of the rules on no match: refused with the text of a value out of range
static int no_match(int what) { return cz_root_rules_order("cz_match", "match", "", what, -1, 0, 0, 0, false); }

int cz_match_set_rules(cz_match *mh, int rules) { return mh ? cz_root_set_rules(mh->root, rules) : no_match(CZ_SET_RULES); }

int cz_match_set_repetition(cz_match *mh, int fold) { return mh ? cz_root_set_repetition(mh->root, fold) : no_match(CZ_SET_REPETITION); }

int cz_match_history(cz_match *mh, const uint64_t **keys, const uint8_t **checks) {
    CZ_REQUIRE(mh, "cz_match_history: cz_match_set_repetition first");
    return cz_root_history(mh->root, keys, checks);
}

int cz_match_set_chase(cz_match *mh, int on) { return mh ? cz_root_set_chase(mh->root, on) : no_match(CZ_SET_CHASE); }

int cz_match_chase_history(cz_match *mh, const uint64_t **chase) {
    CZ_REQUIRE(mh, "cz_match_chase_history: cz_match_set_chase first");
    return cz_root_chase_history(mh->root, chase);
}

int cz_match_set_avoid(cz_match *mh, int on) { return mh ? cz_root_set_avoid(mh->root, on) : no_match(CZ_SET_AVOID); }

int cz_match_avoid_stats(cz_match *mh, int32_t *avoided, int32_t *forced) {
    CZ_REQUIRE(mh, "cz_match_avoid_stats: null match");
    int32_t q[4] = {0, 0, 0, 0};
    CZ_HIP(hipMemcpyAsync(q, mh->m.queue, sizeof(q), hipMemcpyDeviceToHost, mh->a->stream));
    CZ_HIP(hipStreamSynchronize(mh->a->stream));
    if (avoided) *avoided = q[2];
    if (forced) *forced = q[3];
    return CZ_OK;
}

int cz_match_set_resign(cz_match *mh, float threshold, int min_ply) {
    CZ_REQUIRE(mh && min_ply >= 0, "cz_match_set_resign: null match / min_ply < 0");
    mh->m.resign_threshold = threshold;   // NaN: off
    mh->m.resign_min_ply = min_ply;
    return CZ_OK;
}

int cz_match_set_tablebase(cz_match *mh, cz_tb_set *set) {
    CZ_REQUIRE(mh, "cz_match_set_tablebase: null match");
    return cz_root_set_tablebase(mh->root, set);
}

void cz_match_destroy(cz_match *mh) {
    if (!mh) return;
    (void)hipStreamSynchronize(mh->a->stream);
    cz_root_free(mh->root);
    (void)hipFree(mh->block);
    delete mh;
}

int cz_match_active(cz_match *mh, int player, const uint8_t **mask) {
    CZ_REQUIRE(mh && mask && (player == 0 || player == 1), "cz_match_active: player 0 (A) or 1 (B), non-null mask");
    const CzMatch &m = mh->m;
    *mask = player == 0 ? m.act_a : m.act_b;
    return CZ_OK;
}

int cz_match_choose(cz_match *mh, int sample_plies, unsigned long long seed, uint16_t *played) {
    CZ_REQUIRE(mh && played && sample_plies >= 0, "cz_match_choose: null argument / sample_plies < 0");
    CZ_REQUIRE(mh->a->G == mh->G && mh->b->G == mh->G, "cz_match_choose: a context was reset to another number of slots");
    return cz_root_choose(
        mh->root, mh->G, [&] { hipLaunchKernelGGL(k_match_roots_xq, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, mh->m); },
        [&](auto L) {
            hipLaunchKernelGGL(k_match_choose<decltype(L)::value>, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, mh->m, sample_plies, seed,
                               played);
        });
}

int cz_match_adjudicate(cz_match *mh, const uint16_t *played) {
    CZ_REQUIRE(mh && played, "cz_match_adjudicate: null argument");
    CZ_REQUIRE(mh->a->G == mh->G && mh->b->G == mh->G, "cz_match_adjudicate: a context was reset to another number of slots");
    // both trees hold the position after the move (cz_search_advance applies a label to the board of either): the set is probed on A's
    return cz_root_adjudicate(mh->root, played, mh->G, [&](auto L) {
        hipLaunchKernelGGL(k_match_adjudicate<decltype(L)::value>, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, mh->m, played);
    });
}

int cz_match_results(cz_match *mh, const int8_t **result, const uint8_t **a_red, const int32_t **plies, const uint8_t **reason,
                     const uint16_t **moves, const int32_t **slot_game) {
    CZ_REQUIRE(mh, "cz_match_results: null match");
    const CzMatch &m = mh->m;
    if (result) *result = m.result;
    if (a_red) *a_red = m.a_red;
    if (plies) *plies = m.plies;
    if (reason) *reason = m.reason;
    if (moves) *moves = m.moves;
    if (slot_game) *slot_game = m.game;
    return CZ_OK;
}

int cz_match_finished(cz_match *mh, int32_t *finished, unsigned long long *sims) {
    CZ_REQUIRE(mh, "cz_match_finished: null match");
    const CzMatch &m = mh->m;
    int32_t q[2] = {0, 0};
    unsigned long long s = 0ull;
    CZ_HIP(hipMemcpyAsync(q, m.queue, sizeof(q), hipMemcpyDeviceToHost, mh->a->stream));
    CZ_HIP(hipMemcpyAsync(&s, m.sims, sizeof(s), hipMemcpyDeviceToHost, mh->a->stream));
    CZ_HIP(hipStreamSynchronize(mh->a->stream));
    if (finished) *finished = q[1];
    if (sims) *sims = s;
    return CZ_OK;
}
