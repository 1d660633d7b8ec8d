// cz_games.hip — cz_games_replay: G recorded games (move lists) replayed into CZ_REC_* training records in ONE launch.  No
// reference function: the reference learns from its own self-play only (main.py:1493-1554).  One lane = one game, in the frame
// of cz_posframe.h: a wave owns a group of 64 games, stages their start boards once, and every lane keeps ITS board as 23
// packed words in registers across all plies of its game — czg_step (cz_games.h) lists the position's moves with czm_list or
// czk_position, finds the given move in the list and makes it on the words; no board goes back to memory between plies.
// Per ply the wave's 64 records are assembled in LDS, one row of CZG_ROW words per lane (153 = 152 + 1: the 64 lanes' dword
// and halfword stores at the same offset of their rows fall on different banks), and leave as 16-byte stores, 38 contiguous
// pieces per record, consecutive lanes on consecutive pieces of one record.  The generators' scratch has its own 8.5 KB beside
// the rows (czk_position reads it while it puts the list).  A wave runs until its longest game is over: a lane whose game has
// ended or stopped runs along on an empty board (czg_step's go = false) and, while its game still has plies given, writes
// their records as zeros.  The host sorts the games by length, so that a wave's games end together; rec_offset puts the
// records back where the caller wants them.  49.0 KB of LDS per wave: three waves per CU.
#include "cz_internal.h"
#include "cz_games.h"
#include "cz_posframe.h"

static_assert(CZG_OK == CZ_GAME_OK && CZG_ILLEGAL == CZ_GAME_ILLEGAL && CZG_AFTER_END == CZ_GAME_AFTER_END && CZG_BAD_BOARD == CZ_GAME_BAD_BOARD &&
              CZG_BAD_LEN == CZ_GAME_BAD_LEN && CZG_RED_KING_GONE == CZ_GAME_RED_KING_GONE && CZG_BLACK_KING_GONE == CZ_GAME_BLACK_KING_GONE,
              "cz_games.h restates include/cchess_hip.h");
static_assert(CZ_REC_BYTES == 608 && CZ_REC_SIDE == 90 && CZ_REC_COUNT == 91 && CZ_REC_Z == 92 && CZ_REC_PLY == 94 && CZ_REC_LABELS == 96 &&
              CZ_REC_VISITS == 352, "the record layout k_games_replay writes word by word");

namespace {

constexpr int CZG_REC_WORDS = CZ_REC_BYTES / 4;     // 152
constexpr int CZG_ROW = CZG_REC_WORDS + 1;          // words between two lanes' rows in LDS
constexpr int CZG_PIECES = CZ_REC_BYTES / 16;       // 38 pieces of 16 bytes per record

template <int RULES>
__global__ __launch_bounds__(64) void k_games_replay(const CzmTables *__restrict__ gtab, const uint16_t *__restrict__ srcdst,
                                                     const uint8_t *__restrict__ start_boards, const uint8_t *__restrict__ start_side,
                                                     const uint16_t *__restrict__ moves, int stride, const int32_t *__restrict__ len,
                                                     const int8_t *__restrict__ result, int G, const int32_t *__restrict__ rec_offset, int total,
                                                     uint8_t *__restrict__ records, int32_t *__restrict__ valid, uint8_t *__restrict__ status,
                                                     uint8_t *__restrict__ end_flags, uint8_t *__restrict__ final_boards, uint8_t *__restrict__ final_side) {
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
        const uint16_t *const mrow = moves + (size_t)p * (size_t)stride;
        uint32_t label = (!stopped && 0 < n_given) ? mrow[0] : 0xFFFFu;
        for (int i = 0; CZM_ANY(i < n_given); ++i) {
            const bool given = i < n_given, go = given && !stopped;
            const uint32_t next = (go && i + 1 < n_given) ? mrow[i + 1] : 0xFFFFu;   // in flight while this ply is computed
            const uint32_t w22 = w[22];
            if (go) {   // the board BEFORE the move: the step replaces w
#pragma unroll
                for (int k = 0; k < 22; ++k) row[k] = w[k];
            }
            CzgStep r;
            r.n = 0; r.idx = -1; r.status = CZG_ILLEGAL;
            if (CZM_ANY(go)) {   // wave-uniform: a wave whose games have all stopped only writes zero records
                r = czg_step<RULES>(w, sd, label, go, T, srcdst,
                    [&](int k) -> uint32_t & { return slots[k * 64 + lane]; },
                    [lrow](int k, int l) { lrow[k & 127] = (uint16_t)l; },
                    [row]() {
#pragma unroll
                        for (int k = CZ_REC_LABELS / 4; k < CZ_REC_VISITS / 4; ++k) row[k] = 0xFFFFFFFFu;
                    });
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

}  // namespace

int cz_games_replay(cz_ctx *c, const uint8_t *start_boards, const uint8_t *start_side, const uint16_t *moves, int stride, const int32_t *len,
                    const int8_t *result, int G, int rules, const int32_t *rec_offset, int total, uint8_t *records, int32_t *valid,
                    uint8_t *status, uint8_t *end_flags, uint8_t *final_boards, uint8_t *final_side) {
    CZ_REQUIRE(c && G >= 0, "cz_games_replay: null ctx / negative G");
    CZ_REQUIRE(stride >= 0 && stride <= 65535 && total >= 0, "cz_games_replay: 0 <= stride <= 65535 and total >= 0 required");
    CZ_REQUIRE(rules == 0 || rules == 1, "cz_games_replay: rules is 0 (capture) or 1 (king-safe)");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(moves && len && result && rec_offset && valid && status && end_flags,
               "cz_games_replay: moves, len, result, rec_offset, valid, status, end_flags required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15u) == 0, "cz_games_replay: records must be 16-byte aligned");
    CZ_REQUIRE(!final_boards || final_side, "cz_games_replay: final_boards needs final_side");
    const dim3 grid(czf_persistent_grid((G + 63) / 64, 3));   // 49.0 KB of LDS per wave: three waves per CU
#define CZG_LAUNCH(R) hipLaunchKernelGGL((k_games_replay<R>), grid, dim3(64), 0, c->stream, c->mask_tab, c->tab.srcdst, start_boards, start_side, moves, stride, \
                                         len, result, G, rec_offset, total, records, valid, status, end_flags, final_boards, final_side)
    if (rules) CZG_LAUNCH(1);
    else CZG_LAUNCH(0);
#undef CZG_LAUNCH
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
