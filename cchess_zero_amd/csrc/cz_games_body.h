// cz_games_body.h — the body of the replay kernels, once: k_games_replay (cz_games.hip: a ply's move is a uint16 label) and
// k_games_read (cz_notation.hip: a ply's move is a uint32 token, a label or a move named in notation, cz_notation.h).  The
// layout, the phases and their fences are described at the head of cz_games.hip; what the move source Tok changes:
//   uint16_t  czg_step finds the label while the list is put; sdl and labels_out are not used (NULL).
//   uint32_t  bytes 88, 89 of the board go to the row before the step, so that the WHOLE board before the move and the list
//             (the row's label area) are in the lane's LDS row when czn_pick matches the token against the listed moves: the
//             board's 23 words are read back from the row at compile-time places and the labels at run-time indices, so nothing
//             indexes the 23 register words at run time.  sdl is srcdst staged in LDS by
//             the kernel (one 2-byte LDS read per listed move instead of a global one); the step reads it too.  labels_out
//             [G][stride] or NULL: the label every made ply decoded to, 0xFFFF elsewhere — the lane writes its plies given as it
//             goes, the wave fills what lies behind them at the end of the group, so no element is written twice.
#pragma once
#include <type_traits>
#include "cz_internal.h"
#include "cz_games.h"
#include "cz_notation.h"
#include "cz_posframe.h"

constexpr int CZG_REC_WORDS = CZ_REC_BYTES / 4;     // 152
constexpr int CZG_ROW = CZG_REC_WORDS + 1;          // words between two lanes' rows in LDS
constexpr int CZG_PIECES = CZ_REC_BYTES / 16;       // 38 pieces of 16 bytes per record

template <int RULES, typename Tok>
__device__ __forceinline__ void czg_replay_body(const CzmTables *__restrict__ gtab, const uint16_t *srcdst, const uint16_t *sdl,
                                                const uint8_t *__restrict__ start_boards, const uint8_t *__restrict__ start_side,
                                                const Tok *__restrict__ moves, int stride, const int32_t *__restrict__ len,
                                                const int8_t *__restrict__ result, int G, const int32_t *__restrict__ rec_offset, int total,
                                                uint8_t *__restrict__ records, int32_t *__restrict__ valid, uint8_t *__restrict__ status,
                                                uint8_t *__restrict__ end_flags, uint8_t *__restrict__ final_boards, uint8_t *__restrict__ final_side,
                                                uint16_t *__restrict__ labels_out) {
    constexpr bool TOKENS = std::is_same<Tok, uint32_t>::value;
    static_assert(TOKENS || std::is_same<Tok, uint16_t>::value, "a move is a uint16 label or a uint32 token");
    // the 64 start boards (1 440 words + the word lane 63's funnel shift reads behind them), then the 64 record rows; at the
    // end of a group the 64 final boards
    __shared__ __attribute__((aligned(16))) uint32_t rows[64 * CZG_ROW];
    __shared__ uint32_t slots[CZG_SCRATCH * 64];   // [word][lane]
    __shared__ int dsti[64];                       // this ply's record index of every lane's game, or -1: nothing to write
    __shared__ __attribute__((aligned(16))) CzmTables T;
    static_assert(64 * CZG_ROW >= CZF_BOARD_WORDS + 4, "the staged boards fit the rows");
    const int lane = threadIdx.x;
    if (lane < (int)(sizeof(CzmTables) / 16)) reinterpret_cast<uint4 *>(&T)[lane] = reinterpret_cast<const uint4 *>(gtab)[lane];
    uint32_t *const row = rows + lane * CZG_ROW;
    uint16_t *const lrow = reinterpret_cast<uint16_t *>(row + CZ_REC_LABELS / 4);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        const int p = g.g0 + lane;
        CZF_WAVE_FENCE();   // the previous group's rows have left (and the tables are in place)
        uint32_t w[23] = CZG_START_WORDS;
        if (start_boards) {   // wave-uniform
            // the frame's loader wants a side array of G bytes beside the boards; start_side may be NULL, so the loader reads the
            // boards' own first G bytes for it and its answer is dropped
            CzfLoader ld(start_boards, start_boards, G, lane);
            ld.request(grp);
            ld.stage(rows, g);
            CZF_WAVE_FENCE();
            czf_unpack(rows, lane, g.live, w);
            CZF_WAVE_FENCE();   // every lane holds its board: the bytes become record rows
        }
        int sd = (g.live && start_side && start_side[p]) ? 1 : 0;
        const int ln = g.live ? len[p] : 0;
        const bool len_ok = ln >= 0 && ln <= stride;
        const int n_given = len_ok ? ln : 0;
        const long long off = g.live ? (long long)rec_offset[p] : 0ll;
        const int res = g.live ? (int)result[p] : 0;
        int made = 0, st = len_ok ? CZG_OK : CZG_BAD_LEN;
        bool stopped = !g.live || !len_ok;
        const Tok *const mrow = moves + (size_t)p * (size_t)stride;
        uint32_t label = (!stopped && 0 < n_given) ? mrow[0] : 0xFFFFu;
        for (int i = 0; CZM_ANY(i < n_given); ++i) {
            const bool given = i < n_given, go = given && !stopped;
            const uint32_t next = (go && i + 1 < n_given) ? mrow[i + 1] : 0xFFFFu;   // in flight while this ply is computed
            const uint32_t w22 = w[22];
            if (go) {   // the board BEFORE the move: the step replaces w
#pragma unroll
                for (int k = 0; k < 22; ++k) row[k] = w[k];
                if (TOKENS) row[22] = w22;
            }
            CzgStep r;
            r.n = 0; r.idx = -1; r.status = CZG_ILLEGAL;
            uint32_t played = label;   // the label of the move that is made, if one is
            if (CZM_ANY(go)) {   // wave-uniform: a wave whose games have all stopped only writes zero records
                auto scr = [&](int k) -> uint32_t & { return slots[k * 64 + lane]; };
                auto put = [lrow](int k, int l) { lrow[k & 127] = (uint16_t)l; };
                auto mid = [row]() {
#pragma unroll
                    for (int k = CZ_REC_LABELS / 4; k < CZ_REC_VISITS / 4; ++k) row[k] = 0xFFFFFFFFu;
                };
                if constexpr (TOKENS) {
                    const bool text = go && label >= 65536u;
                    // a text token is no label: the step's own search finds nothing (a listed label is < 2086) and the pick decides
                    r = czg_step_pick<RULES>(w, sd, label, go, T, sdl, scr, put, mid, [&](int n, uint32_t &lab, int &idx) {
                        const int miss = czn_pick(label, text, sd, n, lab, idx, [lrow](int j) { return lrow[j & 127]; },
                                                  [sdl](uint32_t l) { return (uint32_t)sdl[l]; }, [row](int k) { return row[k]; });
                        played = lab;
                        return miss;
                    });
                } else {
                    r = czg_step<RULES>(w, sd, label, go, T, srcdst, scr, put, mid);
                }
            }
            const bool rec = go && r.status == CZG_OK;
            if (go && !rec) { stopped = true; st = r.status; }
            // the rest of the record's row.  A made ply: mover, count, z from the mover's side, ply, the list (put above, on the
            // 0xFFFF padding), visits 1 at the played child; a ply given but not made: 608 zero bytes
            if (given) {
                if (rec) {
                    row[22] = czg_rec_word22(w22, sd, r.n);
                    row[23] = czg_rec_word23(sd ? -res : res, i);
#pragma unroll
                    for (int k = CZ_REC_VISITS / 4; k < CZG_REC_WORDS; ++k) row[k] = 0u;
                    reinterpret_cast<uint16_t *>(row + CZ_REC_VISITS / 4)[r.idx & 127] = 1;
                } else {
#pragma unroll
                    for (int k = 0; k < CZG_REC_WORDS; ++k) row[k] = 0u;
                }
                if (TOKENS && labels_out) labels_out[(size_t)p * (size_t)stride + i] = rec ? (uint16_t)played : (uint16_t)0xFFFFu;
            }
            const long long at = off + i;
            dsti[lane] = (given && at >= 0 && at < (long long)total) ? (int)at : -1;
            if (rec) { ++made; sd ^= 1; }
            label = next;
            CZF_WAVE_FENCE();   // the rows are built
            if (records) {
#pragma unroll 2
                for (int k = 0; k < CZG_PIECES; ++k) {   // 64 x 38 pieces, 64 per step: lane l takes piece (l + 64 k) % 38 of row (l + 64 k) / 38
                    const int idx = lane + 64 * k, pp = idx / CZG_PIECES, j = idx - pp * CZG_PIECES;
                    const int d = dsti[pp];
                    if (d >= 0) {
                        const uint32_t *src = rows + pp * CZG_ROW + 4 * j;
                        reinterpret_cast<uint4 *>(records + (size_t)d * CZ_REC_BYTES)[j] = make_uint4(src[0], src[1], src[2], src[3]);
                    }
                }
            }
            CZF_WAVE_FENCE();   // the rows are in registers on their way out
        }
        if (TOKENS && labels_out) {   // behind every game's plies given: 0xFFFF, the wave on one game's row at a time
            for (int pp = 0; pp < g.np; ++pp) {
                const int from = __shfl(n_given, pp, 64);
                uint16_t *const dst = labels_out + (size_t)(g.g0 + pp) * (size_t)stride;
                for (int i = from + lane; i < stride; i += 64) dst[i] = (uint16_t)0xFFFFu;
            }
        }
        // the position the replay reached
        const uint32_t ef = czg_end_flags(w, sd, g.live, T, [&](int k) -> uint32_t & { return slots[k * 64 + lane]; });
        if (g.live) {
            valid[p] = made;
            status[p] = (uint8_t)st;
            end_flags[p] = (uint8_t)ef;
            if (final_side) final_side[p] = (uint8_t)sd;
        }
        if (final_boards) {   // through LDS: the group's 64 boards are 5 760 contiguous bytes
            CZF_WAVE_FENCE();
            uint16_t *const fb = reinterpret_cast<uint16_t *>(rows) + 45 * lane;
#pragma unroll
            for (int k = 0; k < 22; ++k) { fb[2 * k] = (uint16_t)w[k]; fb[2 * k + 1] = (uint16_t)(w[k] >> 16); }
            fb[44] = (uint16_t)w[22];
            CZF_WAVE_FENCE();
            uint8_t *const dst = final_boards + (size_t)g.g0 * CZ_NSQ;
            const int nbytes = g.np * CZ_NSQ;
            if ((reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
                for (int i = lane; i < nbytes / 16; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(rows)[i];
                const int full = nbytes & ~15;
                if (lane < nbytes - full) dst[full + lane] = reinterpret_cast<const uint8_t *>(rows)[full + lane];
            } else {
                for (int i = lane; i < nbytes; i += 64) dst[i] = reinterpret_cast<const uint8_t *>(rows)[i];
            }
        }
    }
}
