// cz_chase.hip — the perpetual-chase rule's two stand-alone calls.
// cz_threats: the chase record of G positions (czc_position, cz_chase.h: the threatened pieces of the side to move and that
// side's squares).  One lane = one position; the frame is the flags-only form of k_movegen_kingsafe (cz_kingsafe.hip): a wave
// stages its 64 boards in LDS, every lane takes its 90 bytes out as 23 dwords, the 17 piece slots of a position live in
// per-position LDS scratch, and a lane's 32 result bytes leave as two 16-byte stores.
// cz_repetition_chase: cz_repetition with the chase verdict behind it (cz_repetition.h: wave_repetition_chase), one wave64 per
// game on records that the caller keeps.
#include "cz_internal.h"
#include "cz_chase.h"
#include "cz_repetition.h"

namespace {

__global__ __launch_bounds__(64) void k_threats(const CzmTables *__restrict__ gtab, const uint8_t *__restrict__ boards,
                                                const uint8_t *__restrict__ side, int G, uint64_t *__restrict__ chase) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[64 * CZ_NSQ / 4 + 4];   // the boards (1 440 words) + the word lane 63's funnel shift reads behind them
    __shared__ uint32_t slots[CZC_SCRATCH * 64];                                  // [word][lane]
    __shared__ __attribute__((aligned(16))) CzmTables T;
    const int lane = threadIdx.x;
    if (lane < (int)(sizeof(CzmTables) / 16)) reinterpret_cast<uint4 *>(&T)[lane] = reinterpret_cast<const uint4 *>(gtab)[lane];
    const int ngroups = (G + 63) >> 6;
    const bool al4 = (reinterpret_cast<uintptr_t>(boards) & 3u) == 0;   // a group starts 5 760 bytes after the last: aligned like the batch
    const bool out16 = (reinterpret_cast<uintptr_t>(chase) & 15u) == 0;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const int g0 = grp * 64, np = min(64, G - g0), p = g0 + lane;
        const bool live = lane < np;
        __syncthreads();   // the previous group's boards have been read (and the tables are in place)
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
        uint64_t out[4];
        czc_position(w, sd, T, [&](int i) -> uint32_t & { return slots[i * 64 + lane]; }, out);
        if (live) {
            uint64_t *dst = chase + (size_t)p * 4;
            if (out16) {
                reinterpret_cast<uint4 *>(dst)[0] = make_uint4((uint32_t)out[0], (uint32_t)(out[0] >> 32), (uint32_t)out[1], (uint32_t)(out[1] >> 32));
                reinterpret_cast<uint4 *>(dst)[1] = make_uint4((uint32_t)out[2], (uint32_t)(out[2] >> 32), (uint32_t)out[3], (uint32_t)(out[3] >> 32));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) dst[k] = out[k];
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_repetition_chase(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check,
                                                         const uint64_t *__restrict__ chase, int stride, const int32_t *__restrict__ len,
                                                         const int32_t *__restrict__ window, const uint8_t *__restrict__ side, int G, int fold,
                                                         uint8_t *__restrict__ verdict, int32_t *__restrict__ first, uint8_t *__restrict__ cause) {
    const int lane = threadIdx.x;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const int L = len[g];
        int v = CZ_REP_NONE, j = -1, why = CZ_CAUSE_NONE;
        if (L >= 1 && L <= stride) {   // a length outside the record answers "no verdict": nothing behind the row is read
            const int n = L - 1;
            const int w = window ? max(0, min(window[g], n)) : n;
            const uint64_t *k = keys + (size_t)g * stride;
            const uint8_t *c = in_check + (size_t)g * stride;
            const uint64_t *r = chase + (size_t)g * stride * 4;
            const uint64_t rec_n[4] = {r[(size_t)n * 4], r[(size_t)n * 4 + 1], r[(size_t)n * 4 + 2], r[(size_t)n * 4 + 3]};
            v = wave_repetition_chase(k, c, r, 0x7fffffff, n, w, k[n], c[n] != 0, rec_n, side[g] ? 1 : 0, fold, lane, j, why);
        }
        if (lane == 0) {
            verdict[g] = (uint8_t)v;
            if (first) first[g] = j;
            if (cause) cause[g] = (uint8_t)why;
        }
    }
}

}  // namespace

int czk_threats(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, uint64_t *chase) {
    if (G == 0) return CZ_OK;
    const int ngroups = (G + 63) / 64, chip = 256 * 12;   // 11.1 KB of LDS per wave: persistent waves walk their groups with a stride
    hipLaunchKernelGGL(k_threats, dim3(ngroups < chip ? ngroups : chip), dim3(64), 0, c->stream, c->mask_tab, boards, side, G, chase);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int czk_repetition_chase(cz_ctx *c, const uint64_t *keys, const uint8_t *in_check, const uint64_t *chase, int stride, const int32_t *len,
                         const int32_t *window, const uint8_t *side, int G, int fold, uint8_t *verdict, int32_t *first, uint8_t *cause) {
    if (G == 0) return CZ_OK;
    hipLaunchKernelGGL(k_repetition_chase, dim3(G < 65536 ? G : 65536), dim3(64), 0, c->stream, keys, in_check, chase, stride, len, window, side,
                       G, fold, verdict, first, cause);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
