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
#include "cz_repetition.h"

struct cz_match {
    cz_ctx *a, *b;
    int G, n_games, max_plies;
    long long pair_base, pair_stride;   // global index of local opening p = pair_base + pair_stride * p (rank sharding)
    void *block;
    int rules;                          // 0: king capture (the reference's games), 1: xiangqi (cz_match_set_rules)
    void *xq_block;                     // rules = 1: the mover's root positions, their king-safe sets and the mated flags
    int fold;                           // 0: no repetition rule, 2..8: a fold-th occurrence ends the game (cz_match_set_repetition)
    void *rep_block;                    // fold != 0: the slots' position rings and verdicts
    bool chosen;                        // a cz_match_choose has run: the repetition rule can no longer be switched on
    int chase;                          // 1: perpetual chase is judged too (cz_match_set_chase; needs fold != 0)
    void *chase_block;                  // chase != 0: the slots' rings of chase records
};

namespace {

// The device view of a match: per slot the game it plays, per game the result.
struct CzMatch {
    int G, n_games, max_plies;
    long long pair_base, pair_stride;
    const uint8_t *open_board;    // [n_games / 2][90]
    const uint8_t *open_side;     // [n_games / 2]
    const int32_t *open_rr;       // [n_games / 2]
    int32_t *queue;               // [2] next game to hand out, games finished
    unsigned long long *sims;     // [1] simulations of the searches whose move was chosen
    int32_t *game;                // [G] game of the slot, -1 = parked
    int32_t *ply;                 // [G] plies played in the slot's game
    uint8_t *mover_a;             // [G] player A is to move in the slot's game
    uint8_t *act_a, *act_b;       // [G] mover masks: this player is to move and the game is live
    uint8_t *stalled;             // [G] the last choose found no root child
    int8_t *result;               // [n_games] +1 / 0 / -1 from A's point of view
    uint8_t *a_red;               // [n_games] 1: A played red
    int32_t *plies;               // [n_games]
    uint8_t *reason;              // [n_games] CZ_MATCH_*
    uint16_t *moves;              // [n_games][max_plies] labels played, 0xFFFF past the end
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the uniform of a sampled move (include/cchess_hip.h cz_match_choose): a pure function of (seed, global game, ply)
__device__ __forceinline__ double match_uniform(unsigned long long seed, long long game, int ply) {
    const unsigned long long h = splitmix64(seed ^ splitmix64(((unsigned long long)game << 16) | (unsigned long long)ply));
    return (double)(h >> 11) * 0x1.0p-53;
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
    if (g == 0 && lane == 0) { m.queue[0] = min(m.G, m.n_games); m.queue[1] = 0; *m.sims = 0ull; }
    take_game(ta, tb, m, g, g, lane);
}

// rules = 1 (cz_match_set_rules): what the xiangqi kernels have beside the match
struct CzMatchXq {
    uint8_t *board;     // [G][90] the mover's root position of every slot (an empty board for a parked slot)
    uint8_t *side;      // [G]
    uint32_t *safe;     // [G][66] its king-safe set (cz_movegen_kingsafe)
    uint8_t *mated;     // [G] the last choose found children, none of them king-safe
};

// fold != 0 (cz_match_set_repetition): the history of every slot's game, a ring over the position index
struct CzMatchRep {
    uint64_t *key;        // [G][64] cz_hash of position i of the slot's game at [i & 63]
    uint8_t *check;       // [G][64] its side to move is in check
    uint8_t *rep;         // [G] CZ_REP_* of the last choose: the game ends by repetition
    uint8_t *flags;       // [G] CZ_POS_* of the mover's root position (cz_movegen_kingsafe)
    uint64_t *root_key;   // [G] its cz_hash
    int fold;
};

// chase != 0 (cz_match_set_chase): the chase record (cz_threats) of every position of the slot's game, a third ring
struct CzMatchChase {
    uint64_t *ring;       // [G][64][4] the record of position i of the slot's game at [i & 63]
    uint64_t *root;       // [G][4] the record of the mover's root position
};
#define CZM_REP_BY_CHASE 0x10   /* in CzMatchRep::rep beside the CZ_REP_* verdict: the loss is a chase, not a perpetual check */

// the first maximum of N over children 0 .. n - 1 (N[r] of child lane + 64 r), wave-uniform: wave_most_visited on registers
__device__ __forceinline__ int wave_first_max(const int N[2], int n, int lane) {
    int bn = -1, bi = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (lane + 64 * r < n && N[r] > bn) { bn = N[r]; bi = lane + 64 * r; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int on = __shfl_xor(bn, d, 64), oi = __shfl_xor(bi, d, 64);
        if (on > bn || (on == bn && oi < bi)) { bn = on; bi = oi; }
    }
    return bi;
}

// get_action of the mover (main.py:1332-1341) on its own tree: greedy, or sampled for the game's first sample_plies plies.
// XQ: among the root children whose move is in the slot's king-safe set — they are compacted, in generation order, and the
// choice runs on the compacted visit counts exactly as it runs on all children under king-capture rules.
// REP (with XQ only): the root position goes into the slot's ring at the game's ply, and a fold-th occurrence inside the last
// min(restrict_round, ply, 63) positions — a capture makes the earlier ones unreachable, and no read leaves the slot's current
// game — ends the game before a move is chosen: no move is logged, the ply stays (k_match_adjudicate_rep)
// CHASE (with REP only): the root position's chase record goes into the slot's third ring the same way, and the verdict is
// wave_repetition_chase's: a repetition that is a draw by checks may be a loss for the side that alone chased one piece
template <bool XQ, bool REP, bool CHASE = false>
__device__ __forceinline__ void choose_on(const CzTrees &t, const CzMatch &m, int g, int game, int sample_plies,
                                          unsigned long long seed, uint16_t *__restrict__ played, int lane, const CzMatchXq &x,
                                          const CzMatchRep &r, const CzMatchChase &c = CzMatchChase{}) {
    if (lane == 0) atomicAdd(m.sims, (unsigned long long)t.sims[g]);
    const TreeView v = view_of(t, g);
    int cb, n;
    root_children(t, g, v, cb, n);
    if (XQ && lane == 0) x.mated[g] = 0;
    if (root_cannot_move(t.status[g], n)) {   // the game is aborted by the adjudication
        if (lane == 0) { played[g] = 0xFFFF; m.stalled[g] = 1; }
        return;
    }
    const int ply = m.ply[g];
    if constexpr (REP) {
        const uint64_t key = r.root_key[g];
        const bool chk = (r.flags[g] & CZ_POS_IN_CHECK) != 0;
        const uint64_t *ring_key = r.key + (size_t)g * 64;
        const uint8_t *ring_check = r.check + (size_t)g * 64;
        if (lane == 0) { r.key[(size_t)g * 64 + (ply & 63)] = key; r.check[(size_t)g * 64 + (ply & 63)] = chk ? 1 : 0; }
        const int w = max(0, min(min(t.root_rr[g], ply), 63));   // entry ply & 63, just written, is never among the w read
        int first, verdict;
        if constexpr (CHASE) {
            uint64_t *ring = c.ring + (size_t)g * 64 * 4;
            const uint64_t rec[4] = {c.root[(size_t)g * 4], c.root[(size_t)g * 4 + 1], c.root[(size_t)g * 4 + 2], c.root[(size_t)g * 4 + 3]};
            if (lane < 4) ring[(ply & 63) * 4 + lane] = c.root[(size_t)g * 4 + lane];   // as the key: never among the positions read below
            int cause;
            verdict = wave_repetition_chase(ring_key, ring_check, ring, 63, ply, w, key, chk, rec, x.side[g] ? 1 : 0, r.fold, lane, first, cause);
            if (cause == CZ_CAUSE_CHASE) verdict |= CZM_REP_BY_CHASE;
        } else {
            verdict = wave_repetition(ring_key, ring_check, 63, ply, w, key, chk, x.side[g] ? 1 : 0, r.fold, lane, first);
        }
        if (verdict != CZ_REP_NONE) {
            if (lane == 0) { played[g] = 0xFFFF; r.rep[g] = (uint8_t)verdict; }
            return;
        }
    }
    int pick;
    if constexpr (XQ) {
        __shared__ int sN[128], sI[128];
        const int ns = wave_kingsafe_children(v, cb, n, x.safe + (size_t)g * CZ_MASK_WORDS, lane, sN, sI);
        if (ns == 0) {   // children, none of them king-safe: checkmate or stalemate, the mover loses (k_match_adjudicate_xq)
            if (lane == 0) { played[g] = 0xFFFF; x.mated[g] = 1; }
            return;
        }
        int N[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) N[r] = lane + 64 * r < ns ? sN[lane + 64 * r] : 0;
        int at;
        if (ply < sample_plies) {
            double pi[2];
            wave_visit_policy(N, ns, 1.0, lane, pi);
            at = wave_pick_inverse_cdf(pi, match_uniform(seed, global_game(m, game), ply), lane);
        } else {
            at = wave_first_max(N, ns, lane);
        }
        pick = sI[at];
    } else if (ply < sample_plies) {
        // select_move -> get_action(state, temperature = 1) (main.py:1123,1433-1435): no Dirichlet noise
        int N[2] = {0, 0};
        double pi[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int i = lane + 64 * r;
            if (i < n) N[r] = v.N[cb + i];
        }
        wave_visit_policy(N, n, 1.0, lane, pi);
        pick = wave_pick_inverse_cdf(pi, match_uniform(seed, global_game(m, game), ply), lane);
    } else {
        pick = wave_most_visited(v, cb, n, lane);
    }
    if (lane == 0) {
        const uint16_t mv = v.move[cb + pick];
        if (ply < m.max_plies) m.moves[(size_t)game * m.max_plies + ply] = mv;
        played[g] = mv;
        m.ply[g] = ply + 1;
    }
}

__global__ __launch_bounds__(64) void k_match_choose(CzTrees ta, CzTrees tb, CzMatch m, int sample_plies, unsigned long long seed,
                                                     uint16_t *__restrict__ played) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) { if (lane == 0) played[g] = 0xFFFF; return; }
    if (m.mover_a[g]) choose_on<false, false>(ta, m, g, game, sample_plies, seed, played, lane, CzMatchXq{}, CzMatchRep{});
    else choose_on<false, false>(tb, m, g, game, sample_plies, seed, played, lane, CzMatchXq{}, CzMatchRep{});
}

// rules = 1, before the choice: the mover's root position of every slot, for cz_movegen_kingsafe
__global__ __launch_bounds__(64) void k_match_roots_xq(CzTrees ta, CzTrees tb, CzMatch m, CzMatchXq x) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const bool live = m.game[g] >= 0;
    const CzTrees &t = m.mover_a[g] ? ta : tb;
    for (int j = lane; j < CZ_NSQ; j += 64) x.board[(size_t)g * CZ_NSQ + j] = live ? t.root_board[(size_t)g * CZD_BOARD_LDS + j] : (uint8_t)0;
    if (lane == 0) x.side[g] = live ? t.root_side[g] : (uint8_t)0;
}
__global__ __launch_bounds__(64) void k_match_choose_xq(CzTrees ta, CzTrees tb, CzMatch m, int sample_plies, unsigned long long seed,
                                                        uint16_t *__restrict__ played, CzMatchXq x) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) { if (lane == 0) played[g] = 0xFFFF; return; }
    if (m.mover_a[g]) choose_on<true, false>(ta, m, g, game, sample_plies, seed, played, lane, x, CzMatchRep{});
    else choose_on<true, false>(tb, m, g, game, sample_plies, seed, played, lane, x, CzMatchRep{});
}
__global__ __launch_bounds__(64) void k_match_choose_rep(CzTrees ta, CzTrees tb, CzMatch m, int sample_plies, unsigned long long seed,
                                                         uint16_t *__restrict__ played, CzMatchXq x, CzMatchRep r) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) { if (lane == 0) played[g] = 0xFFFF; return; }   // a parked slot: before the ring is touched
    if (m.mover_a[g]) choose_on<true, true>(ta, m, g, game, sample_plies, seed, played, lane, x, r);
    else choose_on<true, true>(tb, m, g, game, sample_plies, seed, played, lane, x, r);
}

__global__ __launch_bounds__(64) void k_match_choose_chase(CzTrees ta, CzTrees tb, CzMatch m, int sample_plies, unsigned long long seed,
                                                           uint16_t *__restrict__ played, CzMatchXq x, CzMatchRep r, CzMatchChase c) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) { if (lane == 0) played[g] = 0xFFFF; return; }   // a parked slot: before the rings are touched
    if (m.mover_a[g]) choose_on<true, true, true>(ta, m, g, game, sample_plies, seed, played, lane, x, r, c);
    else choose_on<true, true, true>(tb, m, g, game, sample_plies, seed, played, lane, x, r, c);
}

// After cz_search_advance(played) on both contexts: the follower's failed advance (its root was never expanded, so it has no
// child for the move) is its normal case — it starts a fresh root on the new position; then check_end (main.py:1380-1392)
// plus the match's own endings (ply cap, aborted game), the result, and the slot's next game.
// mated (rules = 1 only, else nullptr): the slot's mover had no king-safe move — CZ_MATCH_MATE, before every other ending
// rep (fold != 0 only, else nullptr): the slot's choose found a fold-th occurrence — CZ_MATCH_REPETITION (a draw) or
// CZ_MATCH_PERPETUAL (the side that checked with every move of the cycle loses), before mate and everything else
// CHASE: rep may carry CZM_REP_BY_CHASE — CZ_MATCH_CHASE, lost by the side that chased, scored like a perpetual check
template <bool XQ, bool REP, bool CHASE = false>
__device__ __forceinline__ void adjudicate_body(const CzTrees &ta, const CzTrees &tb, const CzMatch &m, const uint16_t *__restrict__ played, uint8_t *mated,
                                                uint8_t *rep) {
    const int g = blockIdx.x, lane = threadIdx.x;
    if (g >= m.G) return;
    const int game = m.game[g];
    if (game < 0) return;
    const bool ma = m.mover_a[g] != 0;
    const CzTrees &mv = ma ? ta : tb, &fo = ma ? tb : ta;   // the mover's tree, the follower's
    const bool aborted = m.stalled[g] != 0 || played[g] >= CZ_NLABELS || (mv.status[g] & CZ_ST_BAD_ADVANCE) != 0;
    bool Kmiss, kmiss;
    wave_kings_missing(mv.root_board + (size_t)g * CZD_BOARD_LDS, lane, Kmiss, kmiss);
    const int ply = m.ply[g];
    int reason = 0, verdict = CZ_REP_NONE;
    bool by_chase = false;
    if constexpr (REP) verdict = rep[g];
    if constexpr (CHASE) { by_chase = (verdict & CZM_REP_BY_CHASE) != 0; verdict &= ~CZM_REP_BY_CHASE; }
    if (verdict != CZ_REP_NONE) reason = verdict == CZ_REP_DRAW ? CZ_MATCH_REPETITION : (by_chase ? CZ_MATCH_CHASE : CZ_MATCH_PERPETUAL);
    else if (XQ && mated[g]) reason = CZ_MATCH_MATE;
    else if (aborted) reason = CZ_MATCH_ABORTED;
    else if (Kmiss || kmiss) reason = CZ_MATCH_KING;
    else if (restrict_round_draw(mv.root_rr[g])) reason = CZ_MATCH_RR60;
    else if (ply >= m.max_plies) reason = CZ_MATCH_PLY_CAP;
    if (lane == 0) fo.status[g] &= ~CZ_ST_BAD_ADVANCE;
    if (!reason) {
        if (lane == 0) { m.mover_a[g] = ma ? 0 : 1; m.act_a[g] = ma ? 0 : 1; m.act_b[g] = ma ? 1 : 0; }
        return;
    }
    int next = 0;
    if (lane == 0) {
        const bool a_red = (game & 1) == 0;
        const bool a_wins = (king_capture_winner(Kmiss) == 0) == a_red;
        int8_t result = (int8_t)(reason == CZ_MATCH_KING ? (a_wins ? 1 : -1) : (reason == CZ_MATCH_MATE ? (ma ? -1 : 1) : 0));
        if constexpr (REP) {
            if (reason == CZ_MATCH_PERPETUAL || reason == CZ_MATCH_CHASE) result = (int8_t)(((verdict == CZ_REP_RED_LOSES) == a_red) ? -1 : 1);   // A has the losing colour
        }
        m.result[game] = result;
        if (XQ) mated[g] = 0;
        if constexpr (REP) rep[g] = CZ_REP_NONE;
        m.a_red[game] = a_red ? 1 : 0;
        m.plies[game] = ply;
        m.reason[game] = (uint8_t)reason;
        atomicAdd(&m.queue[1], 1);
        next = atomicAdd(&m.queue[0], 1);
    }
    next = __shfl(next, 0, 64);
    take_game(ta, tb, m, g, next, lane);
}
__global__ __launch_bounds__(64) void k_match_adjudicate(CzTrees ta, CzTrees tb, CzMatch m, const uint16_t *__restrict__ played) {
    adjudicate_body<false, false>(ta, tb, m, played, nullptr, nullptr);
}
__global__ __launch_bounds__(64) void k_match_adjudicate_xq(CzTrees ta, CzTrees tb, CzMatch m, const uint16_t *__restrict__ played, uint8_t *mated) {
    adjudicate_body<true, false>(ta, tb, m, played, mated, nullptr);
}
__global__ __launch_bounds__(64) void k_match_adjudicate_rep(CzTrees ta, CzTrees tb, CzMatch m, const uint16_t *__restrict__ played, uint8_t *mated,
                                                             uint8_t *rep) {
    adjudicate_body<true, true>(ta, tb, m, played, mated, rep);
}
__global__ __launch_bounds__(64) void k_match_adjudicate_chase(CzTrees ta, CzTrees tb, CzMatch m, const uint16_t *__restrict__ played, uint8_t *mated,
                                                               uint8_t *rep) {
    adjudicate_body<true, true, true>(ta, tb, m, played, mated, rep);
}

}  // namespace

// the match's arrays inside its one allocation (base NULL: only the size) -> bytes
static size_t carve(const cz_match *mh, char *base, CzMatch &m) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
    const size_t G = (size_t)mh->G, n = (size_t)mh->n_games, np = n / 2;
    m.G = mh->G; m.n_games = mh->n_games; m.max_plies = mh->max_plies;
    m.pair_base = mh->pair_base; m.pair_stride = mh->pair_stride;
    m.open_board = (const uint8_t *)take(np * CZ_NSQ);
    m.open_side = (const uint8_t *)take(np);
    m.open_rr = (const int32_t *)take(np * 4);
    m.queue = (int32_t *)take(8);
    m.sims = (unsigned long long *)take(8);
    m.game = (int32_t *)take(G * 4);
    m.ply = (int32_t *)take(G * 4);
    m.mover_a = (uint8_t *)take(G);
    m.act_a = (uint8_t *)take(G);
    m.act_b = (uint8_t *)take(G);
    m.stalled = (uint8_t *)take(G);
    m.result = (int8_t *)take(n);
    m.a_red = (uint8_t *)take(n);
    m.plies = (int32_t *)take(n * 4);
    m.reason = (uint8_t *)take(n);
    m.moves = (uint16_t *)take(n * (size_t)mh->max_plies * 2);
    return off;
}

// rules = 1: the arrays of the xiangqi kernels inside their own allocation
static size_t carve_xq(const cz_match *mh, char *base, CzMatchXq &x) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
    const size_t G = (size_t)mh->G;
    x.board = (uint8_t *)take(G * CZ_NSQ);
    x.side = (uint8_t *)take(G);
    x.safe = (uint32_t *)take(G * CZ_MASK_WORDS * 4);
    x.mated = (uint8_t *)take(G);
    return off;
}

// fold != 0: the repetition arrays inside their own allocation
static size_t carve_rep(const cz_match *mh, char *base, CzMatchRep &r) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
    const size_t G = (size_t)mh->G;
    r.key = (uint64_t *)take(G * 64 * 8);
    r.check = (uint8_t *)take(G * 64);
    r.rep = (uint8_t *)take(G);
    r.flags = (uint8_t *)take(G);
    r.root_key = (uint64_t *)take(G * 8);
    r.fold = mh->fold;
    return off;
}

// chase != 0: the chase rings inside their own allocation
static size_t carve_chase(const cz_match *mh, char *base, CzMatchChase &c) {
    size_t off = 0;
    auto take = [&](size_t bytes) { char *q = base ? base + off : nullptr; off += (bytes + 255) & ~(size_t)255; return q; };
    const size_t G = (size_t)mh->G;
    c.ring = (uint64_t *)take(G * 64 * 4 * 8);
    c.root = (uint64_t *)take(G * 4 * 8);
    return off;
}

static CzMatch device_view(const cz_match *mh) {
    CzMatch m;
    carve(mh, (char *)mh->block, m);
    return m;
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
    mh->a = a; mh->b = b; mh->G = a->G; mh->n_games = 2 * n_openings; mh->max_plies = max_plies;
    mh->pair_base = pair_base; mh->pair_stride = pair_stride;
    CzMatch sizing;
    const size_t bytes = carve(mh, nullptr, sizing);
    if (hipMalloc(&mh->block, bytes) != hipSuccess) {
        mh->block = nullptr;
        delete mh;
        cz_set_error("cz_match_create: hipMalloc(%zu B) failed", bytes);
        return CZ_ENOMEM;
    }
    const CzMatch m = device_view(mh);
    const size_t np = (size_t)n_openings;
    int rc = CZ_OK;
    auto fail = [&](hipError_t e, const char *what) {
        cz_set_error("cz_match_create: %s failed: %s", what, hipGetErrorString(e));
        rc = CZ_EHIP;
    };
    hipError_t e;
    if ((e = hipMemsetAsync(mh->block, 0, bytes, a->stream)) != hipSuccess) fail(e, "hipMemsetAsync");
    else if ((e = hipMemsetAsync(m.moves, 0xFF, (size_t)mh->n_games * max_plies * 2, a->stream)) != hipSuccess) fail(e, "hipMemsetAsync");
    else if ((e = hipMemcpyAsync((void *)m.open_board, boards, np * CZ_NSQ, hipMemcpyDeviceToDevice, a->stream)) != hipSuccess) fail(e, "hipMemcpyAsync");
    else if ((e = hipMemcpyAsync((void *)m.open_side, side, np, hipMemcpyDeviceToDevice, a->stream)) != hipSuccess) fail(e, "hipMemcpyAsync");
    else if (rr && (e = hipMemcpyAsync((void *)m.open_rr, rr, np * 4, hipMemcpyDeviceToDevice, a->stream)) != hipSuccess) fail(e, "hipMemcpyAsync");
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

int cz_match_set_rules(cz_match *mh, int rules) {
    CZ_REQUIRE(mh && (rules == 0 || rules == 1), "cz_match_set_rules: rules 0 (king capture) or 1 (xiangqi)");
    CZ_REQUIRE(rules == 1 || mh->fold == 0, "cz_match_set_rules: the repetition rule needs rules 1: cz_match_set_repetition(match, 0) first");
    if (rules == 1 && !mh->xq_block) {
        CzMatchXq sizing;
        const size_t bytes = carve_xq(mh, nullptr, sizing);
        if (hipMalloc(&mh->xq_block, bytes) != hipSuccess) {
            mh->xq_block = nullptr;
            cz_set_error("cz_match_set_rules: hipMalloc(%zu B) failed", bytes);
            return CZ_ENOMEM;
        }
        CZ_HIP(hipMemsetAsync(mh->xq_block, 0, bytes, mh->a->stream));
    }
    mh->rules = rules;
    return CZ_OK;
}

int cz_match_set_repetition(cz_match *mh, int fold) {
    CZ_REQUIRE(mh && (fold == 0 || (fold >= 2 && fold <= 8)), "cz_match_set_repetition: fold 0 (off) or 2..8");
    CZ_REQUIRE(fold == 0 || mh->rules == 1, "cz_match_set_repetition: cz_match_set_rules(match, 1) first (the check flags are the king-safe pass's)");
    CZ_REQUIRE(!mh->chosen,"cz_match_set_repetition: before the first cz_match_choose only (the history starts at the openings)");
    CZ_REQUIRE(fold != 0 || mh->chase == 0, "cz_match_set_repetition: the chase rule needs a fold: cz_match_set_chase(match, 0) first");
    if (fold != 0 && !mh->rep_block) {
        CzMatchRep sizing;
        const size_t bytes = carve_rep(mh, nullptr, sizing);
        if (hipMalloc(&mh->rep_block, bytes) != hipSuccess) {
            mh->rep_block = nullptr;
            cz_set_error("cz_match_set_repetition: hipMalloc(%zu B) failed", bytes);
            return CZ_ENOMEM;
        }
        CZ_HIP(hipMemsetAsync(mh->rep_block, 0, bytes, mh->a->stream));
    }
    mh->fold = fold;
    return CZ_OK;
}

int cz_match_history(cz_match *mh, const uint64_t **keys, const uint8_t **checks) {
    CZ_REQUIRE(mh && mh->fold != 0 && mh->rep_block, "cz_match_history: cz_match_set_repetition first");
    CzMatchRep r;
    carve_rep(mh, (char *)mh->rep_block, r);
    if (keys) *keys = r.key;
    if (checks) *checks = r.check;
    return CZ_OK;
}

int cz_match_set_chase(cz_match *mh, int on) {
    CZ_REQUIRE(mh && (on == 0 || on == 1), "cz_match_set_chase: on 0 or 1");
    CZ_REQUIRE(on == 0 || mh->fold != 0, "cz_match_set_chase: cz_match_set_repetition(match, fold) first (a chase is judged on a repeated position)");
    CZ_REQUIRE(!mh->chosen, "cz_match_set_chase: before the first cz_match_choose only (the history starts at the openings)");
    if (on && !mh->chase_block) {
        CzMatchChase sizing;
        const size_t bytes = carve_chase(mh, nullptr, sizing);
        if (hipMalloc(&mh->chase_block, bytes) != hipSuccess) {
            mh->chase_block = nullptr;
            cz_set_error("cz_match_set_chase: hipMalloc(%zu B) failed", bytes);
            return CZ_ENOMEM;
        }
        CZ_HIP(hipMemsetAsync(mh->chase_block, 0, bytes, mh->a->stream));
    }
    mh->chase = on;
    return CZ_OK;
}

int cz_match_chase_history(cz_match *mh, const uint64_t **chase) {
    CZ_REQUIRE(mh && mh->chase != 0 && mh->chase_block, "cz_match_chase_history: cz_match_set_chase first");
    CzMatchChase c;
    carve_chase(mh, (char *)mh->chase_block, c);
    if (chase) *chase = c.ring;
    return CZ_OK;
}

void cz_match_destroy(cz_match *mh) {
    if (!mh) return;
    (void)hipStreamSynchronize(mh->a->stream);
    (void)hipFree(mh->block);
    if (mh->xq_block) (void)hipFree(mh->xq_block);
    if (mh->rep_block) (void)hipFree(mh->rep_block);
    if (mh->chase_block) (void)hipFree(mh->chase_block);
    delete mh;
}

int cz_match_active(cz_match *mh, int player, const uint8_t **mask) {
    CZ_REQUIRE(mh && mask && (player == 0 || player == 1), "cz_match_active: player 0 (A) or 1 (B), non-null mask");
    const CzMatch m = device_view(mh);
    *mask = player == 0 ? m.act_a : m.act_b;
    return CZ_OK;
}

int cz_match_choose(cz_match *mh, int sample_plies, unsigned long long seed, uint16_t *played) {
    CZ_REQUIRE(mh && played && sample_plies >= 0, "cz_match_choose: null argument / sample_plies < 0");
    CZ_REQUIRE(mh->a->G == mh->G && mh->b->G == mh->G, "cz_match_choose: a context was reset to another number of slots");
    mh->chosen = true;
    if (mh->rules == 1 && mh->fold != 0) {   // as below, with the root positions' check flags and keys for the repetition rule
        CzMatchXq x;
        CzMatchRep r;
        carve_xq(mh, (char *)mh->xq_block, x);
        carve_rep(mh, (char *)mh->rep_block, r);
        hipLaunchKernelGGL(k_match_roots_xq, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), x);
        CZ_HIP(hipGetLastError());
        int rc = czk_movegen_kingsafe(mh->a, x.board, x.side, mh->G, nullptr, nullptr, x.safe, r.flags, 0);
        if (rc != CZ_OK) return rc;
        if ((rc = czk_hash(mh->a, x.board, x.side, mh->G, r.root_key)) != CZ_OK) return rc;
        if (mh->chase) {   // and their chase records, for the third ring
            CzMatchChase c;
            carve_chase(mh, (char *)mh->chase_block, c);
            if ((rc = czk_threats(mh->a, x.board, x.side, mh->G, c.root)) != CZ_OK) return rc;
            hipLaunchKernelGGL(k_match_choose_chase, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), sample_plies, seed, played, x, r, c);
            CZ_HIP(hipGetLastError());
            return CZ_OK;
        }
        hipLaunchKernelGGL(k_match_choose_rep, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), sample_plies, seed, played, x, r);
        CZ_HIP(hipGetLastError());
        return CZ_OK;
    }
    if (mh->rules == 1) {   // the king-safe set of every slot's root position, then the choice among the children in it
        CzMatchXq x;
        carve_xq(mh, (char *)mh->xq_block, x);
        hipLaunchKernelGGL(k_match_roots_xq, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), x);
        CZ_HIP(hipGetLastError());
        const int rc = czk_movegen_kingsafe(mh->a, x.board, x.side, mh->G, nullptr, nullptr, x.safe, nullptr, 0);
        if (rc != CZ_OK) return rc;
        hipLaunchKernelGGL(k_match_choose_xq, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), sample_plies, seed, played, x);
        CZ_HIP(hipGetLastError());
        return CZ_OK;
    }
    hipLaunchKernelGGL(k_match_choose, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), sample_plies, seed, played);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_match_adjudicate(cz_match *mh, const uint16_t *played) {
    CZ_REQUIRE(mh && played, "cz_match_adjudicate: null argument");
    CZ_REQUIRE(mh->a->G == mh->G && mh->b->G == mh->G, "cz_match_adjudicate: a context was reset to another number of slots");
    if (mh->rules == 1 && mh->fold != 0) {
        CzMatchXq x;
        CzMatchRep r;
        carve_xq(mh, (char *)mh->xq_block, x);
        carve_rep(mh, (char *)mh->rep_block, r);
        if (mh->chase) hipLaunchKernelGGL(k_match_adjudicate_chase, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), played, x.mated, r.rep);
        else hipLaunchKernelGGL(k_match_adjudicate_rep, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), played, x.mated, r.rep);
    } else if (mh->rules == 1) {
        CzMatchXq x;
        carve_xq(mh, (char *)mh->xq_block, x);
        hipLaunchKernelGGL(k_match_adjudicate_xq, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), played, x.mated);
    } else {
        hipLaunchKernelGGL(k_match_adjudicate, dim3(mh->G), dim3(64), 0, mh->a->stream, mh->a->t, mh->b->t, device_view(mh), played);
    }
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_match_results(cz_match *mh, const int8_t **result, const uint8_t **a_red, const int32_t **plies, const uint8_t **reason,
                     const uint16_t **moves, const int32_t **slot_game) {
    CZ_REQUIRE(mh, "cz_match_results: null match");
    const CzMatch m = device_view(mh);
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
    const CzMatch m = device_view(mh);
    int32_t q[2] = {0, 0};
    unsigned long long s = 0ull;
    CZ_HIP(hipMemcpyAsync(q, m.queue, sizeof(q), hipMemcpyDeviceToHost, mh->a->stream));
    CZ_HIP(hipMemcpyAsync(&s, m.sims, sizeof(s), hipMemcpyDeviceToHost, mh->a->stream));
    CZ_HIP(hipStreamSynchronize(mh->a->stream));
    if (finished) *finished = q[1];
    if (sims) *sims = s;
    return CZ_OK;
}
