// cz_games.h — one ply of a RECORDED GAME: is the given move legal in the position, which place does it have in the legal
// list, and what is the position after it.  The reference has no such function: its games come from its own search
// (cchess_main.selfplay, main.py:1493-1554) and are never read back.  The rules are the library's own two levels and nothing
// is restated here: level 0 is czm_list (cz_maskgen.h: GameBoard.get_legal_moves' list, main.py:743-1109), level 1 is
// czk_position<LIST> (cz_kingsafe.h: the same list without the moves that leave the mover's king attacked).  One lane owns
// one game, as one lane owns one position there, and the board stays in the lane's 23 packed words from ply to ply: the move
// is made on the words (sim_do_action, main.py:671-672, as k_apply_move makes it on bytes).
// Host-compilable like cz_maskgen.h and cz_kingsafe.h (tests/games_host.cpp): k_games_replay (cz_games.hip) and the host test
// program compile this very text.
#pragma once
#include "cz_kingsafe.h"

// why a game's replay stopped (include/cchess_hip.h: CZ_GAME_*)
#define CZG_OK 0          // every move was made
#define CZG_ILLEGAL 1     // the move is not in the position's list
#define CZG_AFTER_END 2   // a move in a position with a king missing, or (level 1) without a king-safe move
#define CZG_BAD_BOARD 3   // czm_list / czk_position refuse the position (-1)
#define CZG_BAD_LEN 4     // the game's length is outside 0 .. stride
#define CZG_AMBIGUOUS 5   // a notation token names two or more moves of the list (cz_notation.h; cz_games_read only)
// end_flags beside the CZK_* bits (CZ_GAME_*_KING_GONE)
#define CZG_RED_KING_GONE 16u
#define CZG_BLACK_KING_GONE 32u
#define CZG_SCRATCH CZK_SCRATCH   // words of per-game scratch: czk_position's 34 (czm_list takes the first 17)

// the opening position (main.py:585) as the 23 packed words of a board: sq = 9 y + x, four squares per word
#define CZG_START_WORDS                                                                                                          \
    { 0x02040503u, 0x05040201u, 0x00000003u, 0x00000000u, 0x07000000u, 0x00000000u, 0x06000700u, 0x06000600u, 0x06000600u,       \
      0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0x000D0000u, 0x000D000Du, 0x000D000Du, 0x0000000Eu, 0x000E0000u,      \
      0x00000000u, 0x00000000u, 0x0B0C0A00u, 0x0B090809u, 0x00000A0Cu }

// the piece code on square q of the packed board — a select over the 23 words: a register array is never indexed at run time
CZM_FN uint32_t czg_code(const uint32_t (&w)[23], int q) {
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 23; ++k) v = (q >> 2) == k ? w[k] : v;
    return (v >> (8 * (q & 3))) & 0xFFu;
}
// sim_do_action on the words: the piece on `from` goes to `to` (what stood there is taken), `from` is left empty
CZM_FN void czg_apply(uint32_t (&w)[23], int from, int to) {
    const uint32_t pc = czg_code(w, from);
    const uint32_t fm = 0xFFu << (8 * (from & 3)), tm = 0xFFu << (8 * (to & 3)), tv = pc << (8 * (to & 3));
#pragma unroll
    for (int k = 0; k < 23; ++k) {
        uint32_t v = w[k];
        v = (from >> 2) == k ? v & ~fm : v;
        v = (to >> 2) == k ? (v & ~tm) | tv : v;
        w[k] = v;
    }
}
// which kings the board lacks, as end_flags bits
CZM_FN uint32_t czg_kings_gone(const CzmSets &S, int side) {
    const bool own = czm_lowest(S.K) < 0, other = czm_lowest(S.EK) < 0;
    return ((side ? other : own) ? CZG_RED_KING_GONE : 0u) | ((side ? own : other) ? CZG_BLACK_KING_GONE : 0u);
}

// What one ply answers.  status CZG_OK: the move was made (w is the next position), idx is its place in the list; any other
// status: w is unchanged and the game stops here.  n: the length of the list (-1: refused), whatever the status.
struct CzgStep { int n, idx, status; };

// Ply of the game whose position is (w, side), with `label` the move given.  go = false: the lane has no move to make (its
// game is over or has stopped): it runs along on an EMPTY board, so that the wave-wide loops of the generators (CZM_ANY) wait
// for none of its pieces, puts nothing, and answers status CZG_ILLEGAL with n = 0; w is left alone.
//   RULES 0: czm_list's list;  RULES 1: czk_position's king-safe list.
//   scr(i), 0 <= i < CZG_SCRATCH: per-game scratch words;  put(k, label): `label` is move number k < 128 of the list;
//   mid(): called once, before the first put: the place to lay the list's 0xFFFF padding.  The list must not live in the
//   scratch: czk_position still reads its slots while it puts.
//   srcdst[label] = from | to << 8 (cz_tables: label -> squares), read for a move that is made only.
// The order of the tests is the order of CZ_GAME_* in include/cchess_hip.h: a refused board before a missing king before a
// move that is not in the list.
//   czg_step_pick is the same ply with one more hook, for a move that is NAMED against the position instead of given as a label
//   (cz_notation.h): pick(n, label, idx) runs once, when the list of n moves has been put and before the tests; it may replace
//   label and idx (the place in the list, or < 0: none) and answers the status of a move it did not find (CZG_ILLEGAL, or its
//   own).  czg_step is czg_step_pick with a pick that leaves both alone.
template <int RULES, typename Scr, typename Put, typename Mid, typename Pick>
CZM_FN CzgStep czg_step_pick(uint32_t (&w)[23], int side, uint32_t label, bool go, const CzmTables &T, const uint16_t *srcdst, Scr scr, Put put, Mid mid,
                             Pick pick) {
    uint32_t wa[23];
#pragma unroll
    for (int k = 0; k < 23; ++k) wa[k] = go ? w[k] : 0u;
    CzgStep r;
    r.idx = -1;
    if (RULES == 0) {
        r.n = czm_list(wa, side, T,
            [&](int m, int l, uint32_t b) {   // m = 2 (k - 128): czm_list's byte offsets from slot 128
                if (b) {
                    const int k = CZM_IGNORE_SLOT + (m >> 1);
                    put(k, l);
                    r.idx = (uint32_t)l == label ? k : r.idx;
                }
                return m + 2 * (int)b;
            },
            scr, mid, [](int, uint32_t) {});
    } else {
        uint32_t pf;
        r.n = czk_position<true, false>(wa, side, T, scr,
            [&](int k, int l) { put(k, l); r.idx = (uint32_t)l == label ? k : r.idx; },
            [](int, uint32_t) {}, mid, &pf);
    }
    const int miss = pick(r.n, label, r.idx);
    const CzmSets S = czm_sets(wa, side);
    const bool ended = czg_kings_gone(S, side) != 0u || (RULES == 1 && r.n == 0);
    r.status = !go ? CZG_ILLEGAL : r.n < 0 ? CZG_BAD_BOARD : ended ? CZG_AFTER_END : r.idx < 0 ? miss : CZG_OK;
    if (CZM_ANY(r.status == CZG_OK)) {
        const uint32_t sq = r.status == CZG_OK ? srcdst[label] : 0u;   // a listed label is < 2086
        uint32_t wn[23];
#pragma unroll
        for (int k = 0; k < 23; ++k) wn[k] = w[k];
        czg_apply(wn, (int)(sq & 0xFFu), (int)(sq >> 8));
#pragma unroll
        for (int k = 0; k < 23; ++k) w[k] = r.status == CZG_OK ? wn[k] : w[k];
    }
    return r;
}
template <int RULES, typename Scr, typename Put, typename Mid>
CZM_FN CzgStep czg_step(uint32_t (&w)[23], int side, uint32_t label, bool go, const CzmTables &T, const uint16_t *srcdst, Scr scr, Put put, Mid mid) {
    return czg_step_pick<RULES>(w, side, label, go, T, srcdst, scr, put, mid, [](int, uint32_t &, int &) { return CZG_ILLEGAL; });
}

// end_flags of the position a replay reached: cz_movegen_kingsafe's CZ_POS_* bits of it (0 for a board it refuses), at both
// rule levels, and which kings are gone.  live = false: an empty board (see go above), flags 0.
template <typename Scr>
CZM_FN uint32_t czg_end_flags(const uint32_t (&w)[23], int side, bool live, const CzmTables &T, Scr scr) {
    uint32_t wa[23];
#pragma unroll
    for (int k = 0; k < 23; ++k) wa[k] = live ? w[k] : 0u;
    uint32_t pf = 0u;
    czk_position<false, false>(wa, side, T, scr, [](int, int) {}, [](int, uint32_t) {}, []() {}, &pf);
    return live ? pf | czg_kings_gone(czm_sets(wa, side), side) : 0u;
}

// words 22 and 23 of a CZ_REC_* record: board bytes 88, 89, the mover, the count; z, flags = 0, the ply
CZM_FN uint32_t czg_rec_word22(uint32_t w22, int side, int n) { return (w22 & 0xFFFFu) | ((uint32_t)side << 16) | ((uint32_t)n << 24); }
CZM_FN uint32_t czg_rec_word23(int z, int ply) { return ((uint32_t)z & 0xFFu) | ((uint32_t)ply << 16); }
