// cz_kingsafe.hip — cz_movegen_kingsafe: the king-safe moves of G positions (ordered list, count, 2086-bit set) and their
// check flags.  One lane = one position, czk_position (cz_kingsafe.h); the frame around it is k_movegen_list's (cz_rules.hip): a
// wave stages its 64 boards in LDS, every lane takes its 90 bytes out as 23 dwords, and the results leave LDS as rows — first
// the 64 mask rows (each lane ORs its own position's fields into its own row), then, in the same memory, the 64 list rows.
// The 34 scratch words per position of czk_position (the piece slots) have their own 8.5 KB beside the rows.
#include "cz_internal.h"
#include "cz_kingsafe.h"

namespace {

#define CZKS_LROW 65   /* dwords per list row in LDS: 64 + 1 (the lanes' 2-byte stores spread over the banks) */

template <bool LIST, bool SET>
__global__ __launch_bounds__(64) void k_movegen_kingsafe(const CzmTables *__restrict__ gtab, const uint8_t *__restrict__ boards,
                                                         const uint8_t *__restrict__ side, int G, uint16_t *__restrict__ moves,
                                                         uint16_t *__restrict__ count, uint32_t *__restrict__ mask,
                                                         uint8_t *__restrict__ pos_flags, int pad) {
    // the boards (1 440 words + the word lane 63's funnel shift reads behind them), then 64 mask rows, then 64 list rows (4 160
    // words); the flags-only form stages the boards alone: 15.5 instead of 26.6 KB of LDS per wave
    __shared__ __attribute__((aligned(16))) uint32_t rows[(LIST || SET) ? 64 * CZ_MASK_WORDS : 64 * CZ_NSQ / 4 + 4];
    __shared__ uint32_t slots[CZK_SCRATCH * 64];                                  // [word][lane]
    __shared__ __attribute__((aligned(16))) CzmTables T;
    const int lane = threadIdx.x;
    if (lane < (int)(sizeof(CzmTables) / 16)) reinterpret_cast<uint4 *>(&T)[lane] = reinterpret_cast<const uint4 *>(gtab)[lane];
    const int ngroups = (G + 63) >> 6;
    const bool al4 = (reinterpret_cast<uintptr_t>(boards) & 3u) == 0;   // a group starts 5 760 bytes after the last: aligned like the batch
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int g0 = grp * 64, np = min(64, G - g0), p = g0 + lane;
        const bool live = lane < np;
        __syncthreads();   // the previous group's rows have left (and the tables are in place)
        {
            const uint8_t *src = boards + (size_t)g0 * CZ_NSQ;
            const int nbytes = np * CZ_NSQ;
            if (al4) {
                for (int i = lane; i < nbytes / 4; i += 64) rows[i] = reinterpret_cast<const uint32_t *>(src)[i];
                if (lane < (nbytes & 3)) reinterpret_cast<uint8_t *>(rows)[(nbytes & ~3) + lane] = src[(nbytes & ~3) + lane];
            } else {
                for (int i = lane; i < nbytes; i += 64) reinterpret_cast<uint8_t *>(rows)[i] = src[i];
            }
        }
        const int sd = (live && side[p]) ? 1 : 0;
        __syncthreads();
        uint32_t w[23];
        {   // the lane's 90 bytes start at byte 90 * lane: 4-aligned for even lanes, 2 (mod 4) for odd ones
            const int b0 = (CZ_NSQ * lane) >> 2, sh = (lane & 1) * 16;
            uint32_t d[24];
#pragma unroll
            for (int k = 0; k < 24; ++k) d[k] = rows[b0 + k];   // lane 63 reads up to word 1 440: inside rows
#pragma unroll
            for (int k = 0; k < 23; ++k) w[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], (uint32_t)sh);
            w[22] &= 0x0000FFFFu;
            if (!live) {
#pragma unroll
                for (int k = 0; k < 23; ++k) w[k] = 0u;
            }
        }
        __syncthreads();   // every lane holds its board
        if (SET) {
            for (int i = lane; i < 64 * CZ_MASK_WORDS; i += 64) rows[i] = 0u;
            __syncthreads();
        }
        uint32_t pf = 0u;
        uint32_t *const mrow = rows + lane * CZ_MASK_WORDS;
        uint16_t *const lrow = reinterpret_cast<uint16_t *>(rows + lane * CZKS_LROW);
        const int n = czk_position<LIST, SET>(w, sd, T,
            [&](int i) -> uint32_t & { return slots[i * 64 + lane]; },
            [lrow](int k, int label) { lrow[k & 127] = (uint16_t)label; },                                             // k < 128: the slots hold at most 121 moves
            [mrow](int bit, uint32_t f) { czm_or_field([mrow](int wi, uint32_t x) { mrow[wi] |= x; }, bit, f); },     // the lane's own row: wi + 1 <= 65
            [&]() {   // the set is complete: its rows leave, and the same memory becomes the list rows with the ABI's 0xFFFF padding
                if (SET) {
                    __syncthreads();
                    uint32_t *dstm = mask + (size_t)g0 * CZ_MASK_WORDS;
                    if ((reinterpret_cast<uintptr_t>(mask) & 15u) == 0) {   // 64 rows are 1 056 16-byte pieces; a group starts 16 896 bytes after the last
                        for (int i = lane; i < np * CZ_MASK_WORDS / 4; i += 64) reinterpret_cast<uint4 *>(dstm)[i] = reinterpret_cast<const uint4 *>(rows)[i];
                        for (int i = (np * CZ_MASK_WORDS / 4) * 4 + lane; i < np * CZ_MASK_WORDS; i += 64) dstm[i] = rows[i];
                    } else {
                        for (int i = lane; i < np * CZ_MASK_WORDS; i += 64) dstm[i] = rows[i];
                    }
                }
                if (LIST) {
                    __syncthreads();
                    if (pad)
                        for (int i = lane; i < 64 * CZKS_LROW; i += 64) rows[i] = 0xFFFFFFFFu;
                    __syncthreads();
                }
            },
            &pf);
        if (live && count) count[p] = n < 0 ? (uint16_t)0xFFFF : (uint16_t)n;
        if (live && pos_flags) pos_flags[p] = (uint8_t)pf;
        if (LIST) {
            __syncthreads();
            uint4 *dst = reinterpret_cast<uint4 *>(moves + (size_t)g0 * CZD_MAXMOVES);
            for (int k = 0; k < 16; ++k) {   // 64 rows of sixteen 16-byte pieces
                const int idx = lane + 64 * k, pp = idx >> 4, j = idx & 15;
                const int npp = pad ? 128 : __shfl(n, pp, 64);   // a refused position (negative) writes nothing without padding
                if (pp < np && 8 * j < npp) {
                    const uint32_t *src = rows + pp * CZKS_LROW + 4 * j;
                    dst[idx] = make_uint4(src[0], src[1], src[2], src[3]);
                }
            }
        }
    }
}

}  // namespace

int czk_movegen_kingsafe(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, uint16_t *moves, uint16_t *count, uint32_t *mask,
                         uint8_t *pos_flags, int flags) {
    if (G == 0) return CZ_OK;
    if (moves && (reinterpret_cast<uintptr_t>(moves) & 15u)) { cz_set_error("cz_movegen_kingsafe: moves must be 16-byte aligned"); return CZ_EINVAL; }
    const int pad = (flags & CZ_MOVES_NO_PAD) ? 0 : 1;
    const int ngroups = (G + 63) / 64, chip = 256 * ((moves || mask) ? 6 : 10);   // 26.6 / 15.5 KB of LDS per wave: six / ten waves per CU
    const dim3 grid(ngroups < chip ? ngroups : chip);
#define CZKS_LAUNCH(L, S) hipLaunchKernelGGL((k_movegen_kingsafe<L, S>), grid, dim3(64), 0, c->stream, c->mask_tab, boards, side, G, moves, count, mask, pos_flags, pad)
    if (moves && mask) CZKS_LAUNCH(true, true);
    else if (moves) CZKS_LAUNCH(true, false);
    else if (mask) CZKS_LAUNCH(false, true);
    else CZKS_LAUNCH(false, false);
#undef CZKS_LAUNCH
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
