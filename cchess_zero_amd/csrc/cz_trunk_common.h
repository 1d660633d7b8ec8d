// cz_trunk_common.h — what the three one-launch trunk kernels share: k_tower8_c128 (cz_conv_kernel.h), k_trunk_split_c128
// (cz_trunk_split.h) and k_trunk_mx_c128 (cz_trunk_mx.h) were re-tiled from one another.  Here lives, once, what all three use
// and what leaves every kernel's assembly as it was: the weight-ring prologue, the staging of the planes and the per-slab
// bookkeeping of the slab asm.  The live-row clamp, the clock probe, the head-weight staging and the head 1x1 convs are still
// each kernel's own text: as shared functions they change the code around the strict kernels' layer loops, which then measured
// 0.5 - 1.5 % slower (profiles/trunk_common_refactor.md).
// A Geo (T8Geo<P>, XSGeo, MXGeo) names the kernel's LDS layout: THREADS, ROWS, SLAB_BYTES, SLAB_SHIFT, W_OFF, PLANES_OFF.
// Every helper is inlined into its kernel: none of this changes a layer loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace czconv {

// The first three slabs of the ring of four, by LDS-DMA: two 16-byte pieces per lane and slab (voff0 / voff1 = the lane's byte
// offsets inside a slab, wave_u = the wave's number as a scalar).  Prologue only; the loop issues its DMAs from the slab asm.
template <class Geo>
__device__ __forceinline__ void trunk_ring_prologue(unsigned char *smem, const unsigned char *wpk, int nslabs, int wave_u,
                                                    unsigned voff0, unsigned voff1) {
    for (int q = 0; q < 3; ++q) {
        const int slab = q < nslabs ? q : nslabs - 1;
        const unsigned char *src = wpk + (size_t)slab * Geo::SLAB_BYTES;
        unsigned char *dst = smem + Geo::W_OFF + ((unsigned)slab & 3u) * Geo::SLAB_BYTES + (wave_u << 10);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + voff0),
                                         (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + voff1),
                                         (__attribute__((address_space(3))) void *)(dst + Geo::THREADS * 16), 16, 0, 0);
    }
}

// the workgroup's input planes (32 B per cell, natural cell order) into ring buffer 3; rows of positions beyond the batch are zero
template <class Geo>
__device__ __forceinline__ void trunk_stage_planes(unsigned char *smem, const uint16_t *__restrict__ planes, int pos0, int nrows, int tid) {
    const uint4 *g = reinterpret_cast<const uint4 *>(planes + (size_t)pos0 * 90 * 16);
    for (int idx = tid; idx < Geo::ROWS * 2; idx += Geo::THREADS) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (idx < nrows * 2) v = g[idx];
        *reinterpret_cast<uint4 *>(smem + Geo::PLANES_OFF + (idx << 4)) = v;
    }
}

// Per-slab bookkeeping of a slab body (slab g of the launch; WPK = the layer weights as bytes): the LDS addresses of this slab's
// and the next slab's weight fragments (vb, vbn), the global source of slab g + 3 (the last slab again behind the end) and the
// wave's LDS destination of that DMA.  IN_SLOT: declarations of further addresses inside this slab's ring slot (byte offset
// `slot`), placed behind vb — k_trunk_mx_c128's vy and vs; empty for the other two.  Expects vb0, g, nslabs, wave_u and Geo in scope.
#define TRUNK_SLAB_ARGS(WPK, IN_SLOT)                                                                                                 \
    const int slot = ((unsigned)g & 3u) << Geo::SLAB_SHIFT;                                                                           \
    const int vb = vb0 + slot;                                                                                                        \
    IN_SLOT                                                                                                                           \
    const int vbn = vb0 + ((((unsigned)g + 1u) & 3u) << Geo::SLAB_SHIFT);                                                             \
    const int gn = g + 3 < nslabs ? g + 3 : nslabs - 1;                                                                               \
    const unsigned char *sbase = (WPK) + (size_t)gn * Geo::SLAB_BYTES;                                                                \
    const int ldst = Geo::W_OFF + ((((unsigned)g + 3u) & 3u) << Geo::SLAB_SHIFT) + (wave_u << 10);

}  // namespace czconv
