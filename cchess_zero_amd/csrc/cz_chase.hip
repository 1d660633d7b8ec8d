// cz_chase.hip — cz_threats: the chase record of G positions (czc_position, cz_chase.h: the threatened pieces of the side to
// move and that side's squares).  One lane = one position in the frame of cz_posframe.h: a wave stages its 64 boards in LDS (the
// next group's prefetched), every lane takes its 90 bytes out as 23 dwords, the 17 piece slots of a position live in
// per-position LDS scratch, and a lane's 32 result bytes leave as two 16-byte stores.
#include "cz_internal.h"
#include "cz_chase.h"
#include "cz_posframe.h"

namespace {

__global__ __launch_bounds__(64) void k_threats(const CzmTables *__restrict__ gtab, const uint8_t *__restrict__ boards,
                                                const uint8_t *__restrict__ side, int G, uint64_t *__restrict__ chase) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[CZF_BOARD_WORDS + 4];   // the boards + the word lane 63's funnel shift reads behind them
    __shared__ uint32_t slots[CZC_SCRATCH * 64];                                  // [word][lane]
    __shared__ __attribute__((aligned(16))) CzmTables T;
    const int lane = threadIdx.x;
    if (lane < (int)(sizeof(CzmTables) / 16)) reinterpret_cast<uint4 *>(&T)[lane] = reinterpret_cast<const uint4 *>(gtab)[lane];
    const bool out16 = (reinterpret_cast<uintptr_t>(chase) & 15u) == 0;
    CzfLoader ld(boards, side, G, lane);
    ld.request(blockIdx.x);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        CZF_WAVE_FENCE();   // the previous group's boards have been read (and the tables are in place)
        const int sd = ld.stage(rows, g);
        CZF_WAVE_FENCE();
        uint32_t w[23];
        czf_unpack(rows, lane, g.live, w);
        ld.request(grp + gridDim.x);   // in flight while this group is computed
        uint64_t out[4];
        czc_position(w, sd, T, [&](int i) -> uint32_t & { return slots[i * 64 + lane]; }, out);
        if (g.live) {
            uint64_t *dst = chase + (size_t)(g.g0 + lane) * 4;
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

}  // namespace

int cz_threats(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, uint64_t *chase) {
    CZ_REQUIRE(c && G >= 0, "cz_threats: null ctx / negative G");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && chase, "cz_threats: boards, side, chase required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(chase) & 7u) == 0, "cz_threats: chase must be 8-byte aligned");
    // 11.1 KB of LDS per wave: twelve persistent waves per CU
    hipLaunchKernelGGL(k_threats, dim3(czf_persistent_grid((G + 63) / 64, 12)), dim3(64), 0, c->stream, c->mask_tab, boards, side, G, chase);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
