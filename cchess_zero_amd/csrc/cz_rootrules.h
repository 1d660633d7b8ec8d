// cz_rootrules.h — the Xiangqi rules that act at the root of a game slot, shared by the match (cz_match.hip) and self-play
// (cz_selfplay.hip): the king-safe set of the root position, the slot's rings of position keys, check flags and chase records,
// and the repetition / perpetual-check / perpetual-chase verdict on them; and wave_choose_prologue, the steps both choose kernels
// take at a root before they choose.  The search below the root is untouched.  How a game then ends is wave_game_end's
// (cz_internal.h), for these two and the bench driver.  The host side (CzRootHost and its cz_root_* functions) is in cz_internal.h.
#pragma once
#include <type_traits>

#include "cz_device.h"
#include "cz_repetition.h"

// What the rules need per slot, beside the consumer's own game state.  The chase part is an allocation of its own in both
// consumers (NULL while that rule is off).
struct CzRootRules {
    uint8_t *board;         // [G][90] the mover's root position of every slot at the last choose (an empty board for a parked slot)
    uint8_t *side;          // [G]
    uint32_t *safe;         // [G][66] its king-safe set (cz_movegen_kingsafe)
    uint8_t *mated;         // [G] the last choose found children, none of them king-safe
    uint64_t *ring_key;     // [G][64] cz_hash of position i of the slot's game at [i & 63]
    uint8_t *ring_check;    // [G][64] its side to move is in check
    uint8_t *rep;           // [G] CZ_REP_* of the last choose, CZ_REP_BY_CHASE beside it: the game ends by repetition
    uint8_t *flags;         // [G] CZ_POS_* of the root position (cz_movegen_kingsafe)
    uint64_t *root_key;     // [G] its cz_hash
    uint64_t *ring_chase;   // [G][64][4] the chase record (cz_threats) of position i of the slot's game at [i & 63]
    uint64_t *root_chase;   // [G][4] the record of the root position
    int fold;               // 0: no repetition rule, 2..8: a fold-th occurrence ends the game
    // the avoid step (cz_match_set_avoid / cz_selfplay_set_avoid; czv_root_avoid, cz_repmoves.hip): between the root pass and the
    // choose kernel `safe` loses the moves that lose by repetition (cz_repmoves.h), and avoid_sum says what happened
    int avoid;              // 0: off
    int32_t *slot_ply;      // [G] the ply of the slot's game at the last gather, -1 for a parked slot
    int32_t *slot_rr;       // [G] root_rr of the position gathered
    uint8_t *avoid_sum;     // [G] CZ_REPMOVES_* of the last avoid step
};
#define CZ_REP_BY_CHASE 0x10   /* in CzRootRules::rep beside the CZ_REP_* verdict: the loss is a chase, not a perpetual check */

// The rule level of a consumer; every level includes the ones below it.
enum CzRulesLevel {
    CZ_RULES_CAPTURE = 0,      // the reference's games: a king is captured
    CZ_RULES_KINGSAFE = 1,     // moves are king-safe, a mover without one is mated
    CZ_RULES_REPETITION = 2,   // and a fold-th occurrence of the root position ends the game
    CZ_RULES_CHASE = 3,        // and a perpetual chase is judged on it
};
inline int cz_rules_level(int rules, int fold, int chase) {
    return rules != 1 ? CZ_RULES_CAPTURE : (fold == 0 ? CZ_RULES_KINGSAFE : (chase ? CZ_RULES_CHASE : CZ_RULES_REPETITION));
}

// f(std::integral_constant<int, level>): the one place a run-time level picks a kernel instantiation
template <typename F>
inline void cz_by_rules_level(int level, F &&f) {
    switch (level) {
    case CZ_RULES_CHASE: f(std::integral_constant<int, CZ_RULES_CHASE>{}); break;
    case CZ_RULES_REPETITION: f(std::integral_constant<int, CZ_RULES_REPETITION>{}); break;
    case CZ_RULES_KINGSAFE: f(std::integral_constant<int, CZ_RULES_KINGSAFE>{}); break;
    default: f(std::integral_constant<int, CZ_RULES_CAPTURE>{}); break;
    }
}

// Before the choice: slot g's root position of tree set t (CzTrees), for cz_movegen_kingsafe / cz_hash / cz_threats, by one wave64
template <typename Trees>
__device__ __forceinline__ void wave_gather_root(const CzRootRules &rr, const Trees &t, int g, bool live, int ply, int lane) {
    for (int j = lane; j < CZ_NSQ; j += 64) rr.board[(size_t)g * CZ_NSQ + j] = live ? t.root_board[(size_t)g * CZD_BOARD_LDS + j] : (uint8_t)0;
    if (lane == 0) {
        rr.side[g] = live ? t.root_side[g] : (uint8_t)0;
        rr.slot_ply[g] = live ? ply : -1;
        rr.slot_rr[g] = t.root_rr[g];
    }
}
// the avoid step's counters at a ply whose mover chooses among candidates: a move was removed / every move loses
template <typename Count>
__device__ __forceinline__ void root_count_avoid(const CzRootRules &rr, int g, Count count) {
    if (!rr.avoid) return;
    const int s = rr.avoid_sum[g];
    if (s & CZ_REPMOVES_REMOVED) count(0);
    if (s & CZ_REPMOVES_FORCED) count(1);
}

// The root position of slot g's game goes into the slot's rings at the game's ply, and a fold-th occurrence inside the last
// min(root_rr, ply, 63) positions — a capture makes the earlier ones unreachable, and no read leaves the slot's current game —
// ends the game.  CHASE: its chase record goes into the third ring the same way, and the verdict is wave_repetition_chase's: a
// repetition that is a draw by checks may be a loss for the side that alone chased one piece.
// -> CZ_REP_* (| CZ_REP_BY_CHASE), wave-uniform, also left in rr.rep[g] when it is a verdict.  A parked slot never gets here.
template <bool CHASE>
__device__ __forceinline__ int wave_root_history(const CzRootRules &rr, int g, int ply, int root_rr, int lane) {
    const uint64_t key = rr.root_key[g];
    const bool chk = (rr.flags[g] & CZ_POS_IN_CHECK) != 0;
    uint64_t *ring_key = rr.ring_key + (size_t)g * 64;
    uint8_t *ring_check = rr.ring_check + (size_t)g * 64;
    if (lane == 0) { ring_key[ply & 63] = key; ring_check[ply & 63] = chk ? 1 : 0; }
    const int w = max(0, min(min(root_rr, ply), 63));   // entry ply & 63, just written, is never among the w read
    const int side = rr.side[g] ? 1 : 0;
    int first, verdict;
    if constexpr (CHASE) {
        uint64_t *ring = rr.ring_chase + (size_t)g * 64 * 4;
        const uint64_t *root = rr.root_chase + (size_t)g * 4;
        const uint64_t rec[4] = {root[0], root[1], root[2], root[3]};
        if (lane < 4) ring[(ply & 63) * 4 + lane] = root[lane];   // as the key: never among the positions read below
        int cause;
        verdict = wave_repetition_chase(ring_key, ring_check, ring, 63, ply, w, key, chk, rec, side, rr.fold, lane, first, cause);
        if (cause == CZ_CAUSE_CHASE) verdict |= CZ_REP_BY_CHASE;
    } else {
        verdict = wave_repetition(ring_key, ring_check, 63, ply, w, key, chk, side, rr.fold, lane, first);
    }
    if (verdict != CZ_REP_NONE && lane == 0) rr.rep[g] = (uint8_t)verdict;
    return verdict;
}

// What a choose kernel finds at the root of slot g before it chooses, in this order
enum CzRootFound {
    CZ_ROOT_CANDIDATES = 0,   // cb, n, N, at hold the candidates (wave_root_candidates): the consumer chooses among them
    CZ_ROOT_CANNOT_MOVE,      // no child to play (root_cannot_move): the consumer's adjudication aborts the game
    CZ_ROOT_VERDICT,          // from CZ_RULES_REPETITION: the root position ends the game (wave_root_history, left in rr.rep[g])
    CZ_ROOT_MATED,            // from CZ_RULES_KINGSAFE: children, none of them king-safe: checkmate or stalemate
};
// The steps every chooser of a game takes at rule level LEVEL on slot g of tree set t (CzTrees; v = view_of(t, g)), at the
// slot's ply, by one wave64.  From CZ_RULES_KINGSAFE the candidates are the root children whose move is in the slot's king-safe
// set, compacted in generation order, and everything the consumer does with N / at runs on them exactly as it runs on all
// children under king-capture rules.  The consumer's reactions are its own: played[g] = 0xFFFF, its stalled flag and
// rr.mated[g], the moments at which it clears rr.mated / rr.rep, resignation, the record or the move log.
template <int LEVEL, typename Trees, typename View>
__device__ __forceinline__ CzRootFound wave_choose_prologue(const CzRootRules &rr, const Trees &t, const View &v, int g, int ply, int lane,
                                                            int &cb, int &n, int N[2], int at[2]) {
    root_children(t, g, v, cb, n);
    if (root_cannot_move(t, g, n)) return CZ_ROOT_CANNOT_MOVE;
    if constexpr (LEVEL >= CZ_RULES_REPETITION) {
        if (wave_root_history<LEVEL >= CZ_RULES_CHASE>(rr, g, ply, t.root_rr[g], lane) != CZ_REP_NONE) return CZ_ROOT_VERDICT;
    }
    if constexpr (LEVEL >= CZ_RULES_KINGSAFE) {
        __shared__ int sN[128], sI[128];
        n = wave_root_candidates(v, cb, n, rr.safe + (size_t)g * CZ_MASK_WORDS, lane, N, at, sN, sI);
        return n == 0 ? CZ_ROOT_MATED : CZ_ROOT_CANDIDATES;
    } else {
        n = wave_root_candidates(v, cb, n, nullptr, lane, N, at, nullptr, nullptr);
        return CZ_ROOT_CANDIDATES;
    }
}
