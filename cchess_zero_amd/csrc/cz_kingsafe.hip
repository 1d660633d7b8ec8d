// cz_kingsafe.hip — cz_movegen_kingsafe: the king-safe moves of G positions (ordered list, count, 2086-bit set) and their
// check flags.  One lane = one position, czk_position (cz_kingsafe.h), in the frame of cz_posframe.h: a wave stages its 64
// boards in LDS (the next group's prefetched), every lane takes its 90 bytes out as 23 dwords, and the results leave LDS as
// rows — first the 64 mask rows (each lane ORs its own position's fields into its own row), then, in the same memory, the 64
// list rows.  The 34 scratch words per position of czk_position (the piece slots) have their own 8.5 KB beside the rows.
// cz_movegen_checks is the same wave with the second pass of czk_checks: the king-safe moves that give check.
#include "cz_internal.h"
#include "cz_kingsafe.h"
#include "cz_posframe.h"

namespace {

// The body of both kernels below.  CHECKS: czk_position keeps only the king-safe moves that give check (cz_movegen_checks).
template <bool LIST, bool SET, bool CHECKS>
__device__ __forceinline__ void movegen_kingsafe_wave(const CzmTables *__restrict__ gtab, const uint8_t *__restrict__ boards,
                                                      const uint8_t *__restrict__ side, int G, uint16_t *__restrict__ moves,
                                                      uint16_t *__restrict__ count, uint32_t *__restrict__ mask,
                                                      uint8_t *__restrict__ pos_flags, int pad) {
    // the boards (1 440 words + the word lane 63's funnel shift reads behind them), then 64 mask rows, then 64 list rows (4 160
    // words); the flags-only form stages the boards alone: 15.5 instead of 26.6 KB of LDS per wave
    __shared__ __attribute__((aligned(16))) uint32_t rows[(LIST || SET) ? 64 * CZ_MASK_WORDS : CZF_BOARD_WORDS + 4];
    __shared__ uint32_t slots[CZK_SCRATCH * 64];                                  // [word][lane]
    __shared__ __attribute__((aligned(16))) CzmTables T;
    const int lane = threadIdx.x;
    if (lane < (int)(sizeof(CzmTables) / 16)) reinterpret_cast<uint4 *>(&T)[lane] = reinterpret_cast<const uint4 *>(gtab)[lane];
    CzfLoader ld(boards, side, G, lane);
    ld.request(blockIdx.x);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        const int p = g.g0 + lane;
        CZF_WAVE_FENCE();   // the previous group's rows have left (and the tables are in place)
        const int sd = ld.stage(rows, g);
        CZF_WAVE_FENCE();
        uint32_t w[23];
        czf_unpack(rows, lane, g.live, w);
        ld.request(grp + gridDim.x);   // in flight while this group is computed
        CZF_WAVE_FENCE();   // every lane holds its board
        if (SET) {
            for (int i = lane; i < 64 * CZ_MASK_WORDS; i += 64) rows[i] = 0u;
            CZF_WAVE_FENCE();
        }
        uint32_t pf = 0u;
        uint32_t *const mrow = rows + lane * CZ_MASK_WORDS;
        uint16_t *const lrow = reinterpret_cast<uint16_t *>(rows + lane * CZF_LROW);
        const int n = czk_position<LIST, SET, CHECKS>(w, sd, T,
            [&](int i) -> uint32_t & { return slots[i * 64 + lane]; },
            [lrow](int k, int label) { lrow[k & 127] = (uint16_t)label; },                                             // k < 128: the slots hold at most 121 moves
            [mrow](int bit, uint32_t f) { czm_or_field([mrow](int wi, uint32_t x) { mrow[wi] |= x; }, bit, f); },     // the lane's own row: wi + 1 <= 65
            [&]() {   // the set is complete: its rows leave, and the same memory becomes the list rows with the ABI's 0xFFFF padding
                if (SET) {
                    CZF_WAVE_FENCE();
                    czf_store_mask_rows<64>(mask + (size_t)g.g0 * CZ_MASK_WORDS, rows, g.np, lane);
                }
                if (LIST) {
                    CZF_WAVE_FENCE();
                    if (pad)
                        for (int i = lane; i < 64 * CZF_LROW; i += 64) rows[i] = 0xFFFFFFFFu;
                    CZF_WAVE_FENCE();
                }
            },
            &pf);
        if (g.live && count) count[p] = n < 0 ? (uint16_t)0xFFFF : (uint16_t)n;
        if (g.live && pos_flags) pos_flags[p] = (uint8_t)pf;
        if (LIST) {
            CZF_WAVE_FENCE();
            czf_store_list_rows(moves, rows, g, n, pad != 0, lane);
        }
    }
}

template <bool LIST, bool SET>
__global__ __launch_bounds__(64) void k_movegen_kingsafe(const CzmTables *__restrict__ gtab, const uint8_t *__restrict__ boards,
                                                         const uint8_t *__restrict__ side, int G, uint16_t *__restrict__ moves,
                                                         uint16_t *__restrict__ count, uint32_t *__restrict__ mask,
                                                         uint8_t *__restrict__ pos_flags, int pad) {
    movegen_kingsafe_wave<LIST, SET, false>(gtab, boards, side, G, moves, count, mask, pos_flags, pad);
}

// cz_movegen_checks: the same wave with czk_checks behind the filter; no set, so the rows hold the boards and then the list
template <bool LIST>
__global__ __launch_bounds__(64) void k_movegen_checks(const CzmTables *__restrict__ gtab, const uint8_t *__restrict__ boards,
                                                       const uint8_t *__restrict__ side, int G, uint16_t *__restrict__ moves,
                                                       uint16_t *__restrict__ count, uint8_t *__restrict__ pos_flags, int pad) {
    movegen_kingsafe_wave<LIST, false, true>(gtab, boards, side, G, moves, count, nullptr, pos_flags, pad);
}

}  // namespace

int cz_movegen_checks(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves, uint16_t *count, uint8_t *pos_flags,
                      int flags) {
    CZ_REQUIRE(c && G >= 0, "cz_movegen_checks: null ctx / negative G");
    CZ_REQUIRE((flags & ~CZ_MOVES_NO_PAD) == 0, "cz_movegen_checks: unknown flag");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side, "cz_movegen_checks: boards, side required");
    CZ_REQUIRE(moves || count || pos_flags, "cz_movegen_checks: no output requested");
    if (moves && (reinterpret_cast<uintptr_t>(moves) & 15u)) { cz_set_error("cz_movegen_checks: moves must be 16-byte aligned"); return CZ_EINVAL; }
    const int pad = (flags & CZ_MOVES_NO_PAD) ? 0 : 1;
    const dim3 grid(czf_persistent_grid((G + 63) / 64, moves ? 6 : 10));   // the LDS of k_movegen_kingsafe's list / flags-only forms
    if (moves) hipLaunchKernelGGL((k_movegen_checks<true>), grid, dim3(64), 0, c->stream, c->mask_tab, boards, side, G, moves, count, pos_flags, pad);
    else hipLaunchKernelGGL((k_movegen_checks<false>), grid, dim3(64), 0, c->stream, c->mask_tab, boards, side, G, moves, count, pos_flags, pad);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_movegen_kingsafe(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves, uint16_t *count, uint32_t *mask,
                        uint8_t *pos_flags, int flags) {
    CZ_REQUIRE(c && G >= 0, "cz_movegen_kingsafe: null ctx / negative G");
    CZ_REQUIRE((flags & ~CZ_MOVES_NO_PAD) == 0, "cz_movegen_kingsafe: unknown flag");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side, "cz_movegen_kingsafe: boards, side required");
    CZ_REQUIRE(moves || count || mask || pos_flags, "cz_movegen_kingsafe: no output requested");
    if (moves && (reinterpret_cast<uintptr_t>(moves) & 15u)) { cz_set_error("cz_movegen_kingsafe: moves must be 16-byte aligned"); return CZ_EINVAL; }
    const int pad = (flags & CZ_MOVES_NO_PAD) ? 0 : 1;
    const dim3 grid(czf_persistent_grid((G + 63) / 64, (moves || mask) ? 6 : 10));   // 26.6 / 15.5 KB of LDS per wave: six / ten waves per CU
#define CZKS_LAUNCH(L, S) hipLaunchKernelGGL((k_movegen_kingsafe<L, S>), grid, dim3(64), 0, c->stream, c->mask_tab, boards, side, G, moves, count, mask, pos_flags, pad)
    if (moves && mask) CZKS_LAUNCH(true, true);
    else if (moves) CZKS_LAUNCH(true, false);
    else if (mask) CZKS_LAUNCH(false, true);
    else CZKS_LAUNCH(false, false);
#undef CZKS_LAUNCH
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
