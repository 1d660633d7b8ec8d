// cz_conv_kernel.h — N1: the policy/value net trunk as fused MFMA implicit-GEMM kernels (gfx950).
//
// Replaces tf.layers.conv2d(128, 3, 'SAME') + batch_norm(no affine) [+ residual add] + ReLU of the reference
// (policy_value_network.py:45-47, 151-162); BN is folded into the packed weights/bias on the host (net.py).
//
//   k_conv3x3_c128   one conv layer per launch: 4 positions per workgroup, activations loaded once into LDS
//                    for all 9 taps, weights streamed in 32 KB slabs, epilogue through LDS.  Moves 69 KB per
//                    position per layer — the HBM/MFMA balance point — so it is kept as the simple variant
//                    (unit tests); the product path is:
//   k_tower8_c128    first conv + ALL residual blocks + head 1x1 convs in ONE launch, activations resident in
//                    LDS across layers, weights streamed L2 -> LDS by LDS-DMA, hand-scheduled slab loop
//                    (see the block comment in front of it); bf16 or fp16 operands;
//   k_trunk_split_c128  (cz_trunk_split.h) the same launch with every operand split into two 16-bit halves
//                    (three MFMAs per product), and k_trunk_mx_c128 (cz_trunk_mx.h), which folds the two cross terms
//                    into one fp6 MFMA: the strict-precision engines.  cz_trunk_common.h holds what the three
//                    launches share outside their layer loops.
// The measured alternatives of rounds 1-3 (2 positions / 4 waves, one position per wave, two workgroups per CU,
// skewed half-workgroups, ring-free) live in tools/experiments/ — they are not part of the library.
// Common: GEMM view per layer M = B*90 board cells, N = 128, K = 9 taps * 128; v_mfma_f32_32x32x16_bf16 with
// fp32 accumulation; LDS rows of 256 B with the 16-byte chunk c of a row stored at chunk c ^ (row & 15)
// (conflict-free ds_read_b128 fragment reads); weights packed [tap][ci/8][co][ci%8] = the LDS operand image.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cz_trunk_common.h"

namespace czconv {


typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#ifndef CZ_CONV_P
#define CZ_CONV_P 4
#endif
#ifndef CZ_CONV_WAVES_PER_EU
#define CZ_CONV_WAVES_PER_EU 2
#endif
#define CZ_STR_(x) #x
#define CZ_STR(x) CZ_STR_(x)
// ablation switches for tools/conv_ubench.hip (all 0 in the product build)
#ifndef CZ_ABL
#define CZ_ABL 0
#endif
#define CZ_ABL_NO_ACTLOAD 1
#define CZ_ABL_NO_EPILOGUE 2
#define CZ_ABL_NO_MFMA 4
#define CZ_ABL_NO_LDSREAD 8
#define CZ_ABL_NO_WSTREAM 16
constexpr int CV_P = CZ_CONV_P;         // positions per workgroup of the per-layer kernel
constexpr int CV_ROWS = CV_P * 90;      // 360 board cells -> 12 row tiles of 32 (24 rows padding)
constexpr int CV_RT = 3;                // row tiles per wave
constexpr int CV_CT = 2;                // col tiles per wave
constexpr int CV_ROWB = 256;            // bytes per LDS activation row
constexpr int CV_ACT_BYTES = (CV_ROWS + 1) * CV_ROWB;  // + zero row
constexpr int CV_SLAB_BYTES = 128 * 128 * 2;            // 32 KB: one whole tap
constexpr int CV_LDS_BYTES = CV_ACT_BYTES + 2 * CV_SLAB_BYTES;
constexpr int CV_THREADS = 128 * CV_P;  // CV_P row groups x 2 column groups of waves
constexpr int CV_PRE = (CV_SLAB_BYTES / 16) / CV_THREADS;  // uint4 prefetch registers per thread

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {  // round to nearest even; NaN stays NaN
    const uint32_t u = __float_as_uint(f);
    const uint32_t r = u + 0x7FFFu + ((u >> 16) & 1u);
    const bool nan = (u & 0x7FFFFFFFu) > 0x7F800000u;
    return (uint16_t)((nan ? (u | 0x400000u) : r) >> 16);
}

// in/out/res: [B][90][128] bf16 (NHWC with H*W = 90).  wpk: [9 taps][16 kchunks][128 n][8] bf16.
__global__ __launch_bounds__(CV_THREADS, CZ_CONV_WAVES_PER_EU) void k_conv3x3_c128(const uint16_t *__restrict__ in,
                                                             const uint16_t *__restrict__ wpk,
                                                             const float *__restrict__ bias,
                                                             const uint16_t *__restrict__ res,
                                                             uint16_t *__restrict__ out, int B, int relu) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char *act = smem;
    unsigned char *wbuf = smem + CV_ACT_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, khalf = lane >> 5;
    const int pos0 = blockIdx.x * CV_P;
    const int npos = (B - pos0) < CV_P ? (B - pos0) : CV_P;
    const int nrows = npos * 90;

    // ---- stage activations: contiguous 16-byte chunks, swizzled rows ----
    {
        const uint4 *g = reinterpret_cast<const uint4 *>(in + (size_t)pos0 * 90 * 128);
        for (int idx = tid; idx < CV_ROWS * 16; idx += CV_THREADS) {
            const int r = idx >> 4, c = idx & 15;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (!(CZ_ABL & CZ_ABL_NO_ACTLOAD) && r < nrows) v = g[idx];
            *reinterpret_cast<uint4 *>(act + r * CV_ROWB + ((c ^ (r & 15)) << 4)) = v;
        }
        if (tid < 16) *reinterpret_cast<uint4 *>(act + CV_ROWS * CV_ROWB + (tid << 4)) = make_uint4(0, 0, 0, 0);
    }
    // ---- slab 0 of the weights ----
    const uint4 *wg = reinterpret_cast<const uint4 *>(wpk);
    // prefetch registers as named scalars (an indexed array here ends up in scratch memory)
    static_assert(CV_PRE == 4, "slab prefetch is written for 4 x 16 B per thread");
#define CV_LD(q) uint4 pre##q = wg[tid + q * CV_THREADS];
#define CV_ST(q, base) *reinterpret_cast<uint4 *>((base) + ((tid + q * CV_THREADS) << 4)) = pre##q;
    CV_LD(0) CV_LD(1) CV_LD(2) CV_LD(3)
    CV_ST(0, wbuf) CV_ST(1, wbuf) CV_ST(2, wbuf) CV_ST(3, wbuf)
    __syncthreads();

    // per-lane geometry of the 3 row tiles this wave owns
    int hh[CV_RT], ww[CV_RT], rown[CV_RT];
#pragma unroll
    for (int i = 0; i < CV_RT; ++i) {
        const int r = 32 * (wr * CV_RT + i) + l31;
        rown[i] = r;
        const int pix = r % 90;
        hh[i] = pix / 10;
        ww[i] = pix - hh[i] * 10;
        if (r >= CV_ROWS) hh[i] = -100;  // padding rows: every tap invalid -> zero row
    }
    const int bcol = (wc * 64 + l31) << 4;  // byte offset of this lane's column inside a kchunk row group

    f32x16 acc[CV_RT][CV_CT];
#pragma unroll
    for (int i = 0; i < CV_RT; ++i)
#pragma unroll
        for (int j = 0; j < CV_CT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

#pragma unroll 1
    for (int s = 0; s < 9; ++s) {
        const int tap = s;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        if (!(CZ_ABL & CZ_ABL_NO_WSTREAM) && s + 1 < 9) {  // issue-early: next slab to registers
            const uint4 *wn = wg + (s + 1) * (CV_SLAB_BYTES / 16) + tid;
            pre0 = wn[0]; pre1 = wn[CV_THREADS]; pre2 = wn[2 * CV_THREADS]; pre3 = wn[3 * CV_THREADS];
        }
        int abase[CV_RT], asw[CV_RT];
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) {
            const int y = hh[i] + dy, x = ww[i] + dx;
            const bool ok = (y >= 0) && (y < 9) && (x >= 0) && (x < 10);
            const int rr = ok ? rown[i] + dy * 10 + dx : CV_ROWS;
            abase[i] = rr * CV_ROWB;
            asw[i] = rr & 15;
        }
        const unsigned char *wb = wbuf + (s & 1) * CV_SLAB_BYTES;
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
            const int c = kk * 2 + khalf;  // 16-byte chunk (8 channels) of the activation row
            bf16x8 a[CV_RT], b[CV_CT];
#pragma unroll
            for (int i = 0; i < CV_RT; ++i) {
                if (CZ_ABL & CZ_ABL_NO_LDSREAD) { for (int e = 0; e < 8; ++e) a[i][e] = (__bf16)(float)(abase[i] + e + c); }
                else a[i] = *reinterpret_cast<const bf16x8 *>(act + abase[i] + ((c ^ asw[i]) << 4));
            }
#pragma unroll
            for (int j = 0; j < CV_CT; ++j) {
                if (CZ_ABL & CZ_ABL_NO_LDSREAD) { for (int e = 0; e < 8; ++e) b[j][e] = (__bf16)(float)(bcol + e + kk + j); }
                else b[j] = *reinterpret_cast<const bf16x8 *>(wb + (kk * 2 + khalf) * 2048 + bcol + j * 512);
            }
#pragma unroll
            for (int i = 0; i < CV_RT; ++i)
#pragma unroll
                for (int j = 0; j < CV_CT; ++j) {
                    if (CZ_ABL & CZ_ABL_NO_MFMA) { asm volatile("" :: "v"(a[i]), "v"(b[j])); acc[i][j][0] += 1.0f; }
                    // weights as the MFMA "A" operand: D[channel][cell] -> a lane owns 4 consecutive channels
                    // of one board cell per accumulator quad, which the epilogue packs into 8-byte stores
                    else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
                }
        }
        if (!(CZ_ABL & CZ_ABL_NO_WSTREAM) && s + 1 < 9) {  // write-late: the other slab buffer was last read in iteration s-1
            unsigned char *nb = wbuf + ((s + 1) & 1) * CV_SLAB_BYTES;
            CV_ST(0, nb) CV_ST(1, nb) CV_ST(2, nb) CV_ST(3, nb)
        }
        __syncthreads();
    }

    if (CZ_ABL & CZ_ABL_NO_EPILOGUE) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < CV_RT; ++i)
#pragma unroll
            for (int j = 0; j < CV_CT; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) t += acc[i][j][e];
        if (t == 12345.678f) out[tid] = 1;  // keeps the accumulators live without the store pass
        return;
    }
    // ---- epilogue: bias (+ residual) (+ ReLU) -> bf16, through LDS, full-row stores ----
    // After the last barrier nobody reads `act` any more: reuse it as the [360][128] bf16 output tile
    // (same swizzle, so the row-wise read-back below is conflict free as well).
#pragma unroll
    for (int i = 0; i < CV_RT; ++i) {
        const int r = 32 * (wr * CV_RT + i) + l31;  // board cell (row of the NHWC matrix) this lane owns
        if (r < CV_ROWS) {
#pragma unroll
            for (int j = 0; j < CV_CT; ++j) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n0 = wc * 64 + j * 32 + 8 * q + 4 * khalf;  // 4 consecutive output channels
                    const float4 bq = *reinterpret_cast<const float4 *>(bias + n0);
                    float v0 = acc[i][j][4 * q + 0] + bq.x, v1 = acc[i][j][4 * q + 1] + bq.y;
                    float v2 = acc[i][j][4 * q + 2] + bq.z, v3 = acc[i][j][4 * q + 3] + bq.w;
                    if (relu && !res) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f); }
                    uint2 pk;
                    pk.x = (uint32_t)f32_to_bf16(v0) | ((uint32_t)f32_to_bf16(v1) << 16);
                    pk.y = (uint32_t)f32_to_bf16(v2) | ((uint32_t)f32_to_bf16(v3) << 16);
                    *reinterpret_cast<uint2 *>(act + r * CV_ROWB + (((n0 >> 3) ^ (r & 15)) << 4) + ((n0 & 4) << 1)) = pk;
                }
            }
        }
    }
    __syncthreads();
    {
        uint4 *go = reinterpret_cast<uint4 *>(out + (size_t)pos0 * 90 * 128);
        const uint4 *gr = res ? reinterpret_cast<const uint4 *>(res + (size_t)pos0 * 90 * 128) : nullptr;
        for (int idx = tid; idx < nrows * 16; idx += CV_THREADS) {
            const int r = idx >> 4, c = idx & 15;
            uint4 v = *reinterpret_cast<const uint4 *>(act + r * CV_ROWB + ((c ^ (r & 15)) << 4));
            if (gr) {
                const uint4 q = gr[idx];
                uint32_t vv[4] = {v.x, v.y, v.z, v.w}, qq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float lo = bf16_to_f32((uint16_t)(vv[t] & 0xFFFF)) + bf16_to_f32((uint16_t)(qq[t] & 0xFFFF));
                    float hi = bf16_to_f32((uint16_t)(vv[t] >> 16)) + bf16_to_f32((uint16_t)(qq[t] >> 16));
                    if (relu) { lo = fmaxf(lo, 0.f); hi = fmaxf(hi, 0.f); }
                    vv[t] = (uint32_t)f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
                }
                v = make_uint4(vv[0], vv[1], vv[2], vv[3]);
            }
            go[idx] = v;
        }
    }
}

constexpr int TW_NBUF = 4;                         // LDS weight ring: four slabs
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {  // one v_cvt_pk_bf16_f32 (RNE)
    f32x2 v; v[0] = lo; v[1] = hi;
    bf16x2 b = __builtin_convertvector(v, bf16x2);
    return *reinterpret_cast<uint32_t *>(&b);
}

struct TwFrag { bf16x8 a[CV_RT]; bf16x8 b[CV_CT]; };

#include "cz_tower_slab_asm.inc"

// the five fragment reads of one k-step, no MFMAs (layer prologue)
#define TW_LOADSET(CA, OB0, OB1, X, AB, KEY, VB)                                                     \
    asm volatile(                                                                                    \
        "v_xor_b32 %[t0], " #CA ", %[k0]\n\t"                                                        \
        "v_xor_b32 %[t1], " #CA ", %[k1]\n\t"                                                        \
        "v_xor_b32 %[t2], " #CA ", %[k2]\n\t"                                                        \
        "v_lshl_add_u32 %[t0], %[t0], 4, %[b0]\n\t"                                                  \
        "v_lshl_add_u32 %[t1], %[t1], 4, %[b1]\n\t"                                                  \
        "v_lshl_add_u32 %[t2], %[t2], 4, %[b2]\n\t"                                                  \
        "ds_read_b128 %[xa0], %[t0]\n\t"                                                             \
        "ds_read_b128 %[xa1], %[t1]\n\t"                                                             \
        "ds_read_b128 %[xa2], %[t2]\n\t"                                                             \
        "ds_read_b128 %[xb0], %[vb] offset:" #OB0 "\n\t"                                             \
        "ds_read_b128 %[xb1], %[vb] offset:" #OB1 "\n\t"                                             \
        : [xa0] "=&v"(X.a[0]), [xa1] "=&v"(X.a[1]), [xa2] "=&v"(X.a[2]), [xb0] "=&v"(X.b[0]),         \
          [xb1] "=&v"(X.b[1]), [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2)                          \
        : [k0] "v"(KEY[0]), [k1] "v"(KEY[1]), [k2] "v"(KEY[2]), [b0] "v"(AB[0]), [b1] "v"(AB[1]),      \
          [b2] "v"(AB[2]), [vb] "v"(VB)                                                               \
        : "memory")


// =================================================================================================
// k_tower8_c128: the same one-launch net trunk with FOUR positions per workgroup and EIGHT waves (two per SIMD).
//
// The accumulators of the 8 waves hold a layer's complete output (360 cells x 128 channels), so a layer can be
// written back IN PLACE once every wave has finished reading its input: only one activation buffer U (90 KB for
// 4 positions) is needed instead of U and V.  The block input x needed by the residual add is kept by each lane
// in registers (48 packed bf16 pairs) and folded into the accumulator initialisation of the block's second conv.
// Compared with k_tower_c128 this halves the L2 -> LDS weight stream per position and gives every SIMD a second
// wave that issues MFMAs while the first one waits, loads or runs its epilogue.
//   waves   8 = 4 (row groups of 3 tiles) x 2 (column groups of 2 tiles); 3x2 accumulators each; <= 256 registers.
//   frags   two register sets; each k-step waits for its own set, then interleaves its 6 MFMAs with the reads of
//           the next k-step.
//   weights same 4-deep ring of 16 KB slabs by LDS-DMA, 2 pieces per wave and slab, counted vmcnt(2).
//   layer   main loop -> s_barrier (all reads of U done) -> epilogue writes U in place -> s_barrier.
// (A P = 2 instance with two workgroups per CU — "2x" — measured the same and was removed; tools/experiments/.)
// =================================================================================================
// Geometry of the kernel: P = 4 positions per workgroup, eight waves, one workgroup per CU, 16 KB slabs.
template <int P> struct T8Geo {
    static_assert(P == 4, "k_tower8_c128 is built for 4 positions per workgroup");
    static constexpr int ROWS = P * 90;                        // 360 cells -> 12 row tiles of 32
    static constexpr int THREADS = P * 128;                    // 2 waves per position: 3 x 2 accumulator tiles each
    static constexpr int SLAB_BYTES = 64 * 128 * 2;            // 64 input channels of one tap
    static constexpr int SLAB_SHIFT = 14;
    static constexpr int SLABS_PER_LAYER = 9 * 128 * 128 * 2 / SLAB_BYTES;    // 18
    static constexpr int ZERO_OFF = ROWS * CV_ROWB;            // 92,160
    static constexpr int W_OFF = ZERO_OFF + CV_ROWB;
    static constexpr int LDS_BYTES = W_OFF + TW_NBUF * SLAB_BYTES;            // 157,952
    static constexpr int PLANES_OFF = W_OFF + 3 * SLAB_BYTES;  // the input planes (32 B per cell) borrow ring buffer 3
    static constexpr int HEADW_OFF = LDS_BYTES;                // head 1x1 conv weights [3][128] f32, staged at the prologue
    static constexpr int LDS_TOTAL = LDS_BYTES + 3 * 128 * 4;  // 159,488 of the CU's 163,840
};
constexpr int T8_P = 4, T8_THREADS = T8Geo<4>::THREADS, T8_LDS_BYTES = T8Geo<4>::LDS_TOTAL;
constexpr int T8_ROWS = T8Geo<4>::ROWS, T8_ZERO_OFF = T8Geo<4>::ZERO_OFF, T8_W_OFF = T8Geo<4>::W_OFF, T8_PLANES_OFF = T8Geo<4>::PLANES_OFF;

// Element type of activations and weights: bf16 (F16 = false) or IEEE fp16 (F16 = true, the reference's
// "19-block fp16" configuration); accumulation is fp32 either way and only the MFMA opcode, the pack / unpack
// conversions and the plane encoding's 1.0 differ.
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <bool F16> __device__ __forceinline__ f32x2 unpack_pair(uint32_t u) {
    if constexpr (F16) return __builtin_convertvector(__builtin_bit_cast(f16x2, u), f32x2);
    else return f32x2{__uint_as_float(u << 16), __uint_as_float(u & 0xFFFF0000u)};
}
template <bool F16> __device__ __forceinline__ uint32_t pack_pair(f32x2 v) {   // round to nearest even
    if constexpr (F16) return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2));
    else return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
template <bool F16> __device__ __forceinline__ f32x16 mfma_32x32x16(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// Measurement only (tools/tower_ubench.hip built with -DCZ_T8_TRACE=1|2; never defined in the library): lane 0 of every wave
// writes the shader clock at fixed points of every layer — 0 layer top, 1 operands of the first k-step requested, 2 main loop
// drained (in front of the "all reads of U done" barrier), 3 epilogue stored and published; with CZ_T8_TRACE=2 also 4..12 after
// each tap (this waits for the scalar unit inside the software-pipelined loop: perturbs it, read as an upper bound).
#if defined(CZ_T8_TRACE)
__device__ unsigned long long *cz_t8_trace_buf;   // [workgroup][wave][layer][16]
#define CZ_T8_STAMP(K)                                                                                               \
    do {                                                                                                             \
        const unsigned long long ts_ = __builtin_readcyclecounter();                                                 \
        if (lane == 0) cz_t8_trace_buf[(((size_t)blockIdx.x * (P * 2) + wave_u) * nlayers + layer) * 16 + (K)] = ts_; \
    } while (0)
#else
#define CZ_T8_STAMP(K)
#endif

template <bool F16, int P>
__global__ __launch_bounds__(P * 128, 2) void k_tower8_c128(const uint16_t *__restrict__ in,
                                                               const uint16_t *__restrict__ wpk,
                                                               const float *__restrict__ bias,
                                                               uint16_t *__restrict__ out,
                                                               const float *__restrict__ head_w,
                                                               const float *__restrict__ head_b,
                                                               float *__restrict__ head_out,
                                                               const uint16_t *__restrict__ planes,
                                                               const uint16_t *__restrict__ w0,
                                                               const float *__restrict__ b0,
                                                               int B, int nlayers,
                                                               const int *__restrict__ bcount,    // device row count or NULL
                                                               unsigned long long *__restrict__ clk) {   // clock probe [grid][4] or NULL (cz_set_clock_probe)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using Geo = T8Geo<P>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, khalf = lane >> 5;
    const int pos0 = blockIdx.x * P;
    if (bcount) {   // compact batches: only the first *bcount rows are live this step (whole workgroups beyond them leave)
        const int live = *bcount;
        B = live < B ? live : B;
    }
    if (pos0 >= B) return;
    // measurement hook (bench.py roofline.effective_clock_GHz): workgroup lifetime in shader-clock cycles (s_memtime) and in
    // the constant 100 MHz reference clock (s_memrealtime); four scalar registers, one uniform branch when the probe is off
    unsigned long long clk_c0 = 0, clk_r0 = 0;
    if (clk) { clk_c0 = __builtin_readcyclecounter(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
    const int npos = (B - pos0) < P ? (B - pos0) : P;
    const int nrows = npos * 90;
    const int nslabs = nlayers * Geo::SLABS_PER_LAYER;
    const unsigned voff0 = (unsigned)tid << 4, voff1 = voff0 + (unsigned)Geo::THREADS * 16u;   // second DMA piece of a slab
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // Cell order inside the workgroup (round 4): the 384 GEMM rows are the 24 padding rows, then the 360 cells of the
    // four positions TILED BY BORDER CLASS, so that whole 32-row tiles are off the board for a tap and their MFMAs are not issued:
    //   LDS rows   0 ..  39  rank 0 (y = 0): (p, x = 8, 9) x 4, then (p, x = 0..7) x 4      GEMM tiles 0 (with the padding), 1
    //             40 ..  71  file 0 (x = 0), ranks 1..8: 8 p + (y - 1)                      tile 2   "left":   dx = -1 taps
    //             72 .. 103  rank 8 (y = 8), files 1..8: 8 p + (x - 1)                      tile 3   "bottom": dy = +1 taps
    //            104 .. 167  interior cells j = 56 p + 8 (y - 1) + (x - 1), j < 64           tiles 4, 5
    //            168 .. 199  file 9 (x = 9), ranks 1..8                                     tile 6   "right":  dx = +1 taps
    //            200 .. 359  interior cells j >= 64                                          tiles 7 .. 11
    // A cell group (two waves) owns the tiles wr, wr + 4, wr + 8, so per tap the skippable tiles of the wave pair on SIMDs 0 / 1
    // (groups 0, 2: top, left, right) and of the pair on SIMDs 2 / 3 (groups 1, 3: top, bottom) balance in taps 0, 1, 2, 6, 8.
    // The order being arbitrary, a cell's 16-byte-chunk swizzle key is no longer its row & 15 but 8 ((y + p) & 1) + ((x + y) & 7):
    // the 16 lanes of every ds_read_b128 group (two board rows of eight cells, or sixteen cells of one file of two positions) hit
    // 16 distinct slots for every tap (emulated: tools/experiments/trunk_layout_emulation.py; the 8 rank-0 cells that share tile 0
    // with the padding are the exception: 2-way).
    auto row_of = [](int p, int y, int x) -> int {
        if (y == 0) return x < 8 ? 8 + 8 * p + x : 2 * p + (x - 8);
        if (x == 0) return 40 + 8 * p + (y - 1);
        if (x == 9) return 168 + 8 * p + (y - 1);
        if (y == 8) return 72 + 8 * p + (x - 1);
        const int j = 56 * p + 8 * (y - 1) + (x - 1);
        return j < 64 ? 104 + j : 136 + j;
    };
    auto key_of = [](int p, int y, int x) -> int { return 8 * ((y + p) & 1) + ((x + y) & 7); };
    auto lds_of_natural = [&](int natural, int c) -> int {   // natural = p * 90 + y * 10 + x; byte offset of 16-byte chunk c of the cell's row
        const int p = natural / 90, cc = natural - p * 90, y = cc / 10, x = cc - y * 10;
        return row_of(p, y, x) * CV_ROWB + ((c ^ key_of(p, y, x)) << 4);
    };

    trunk_ring_prologue<Geo>(smem, reinterpret_cast<const unsigned char *>(wpk), nslabs, wave_u, voff0, voff1);
    if (planes == nullptr) {
        const uint4 *g = reinterpret_cast<const uint4 *>(in + (size_t)pos0 * 90 * 128);
        for (int idx = tid; idx < Geo::ROWS * 16; idx += Geo::THREADS) {
            const int r = idx >> 4, c = idx & 15;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (r < nrows) v = g[idx];
            *reinterpret_cast<uint4 *>(smem + lds_of_natural(r, c)) = v;
        }
    } else {
        trunk_stage_planes<Geo>(smem, planes, pos0, nrows, tid);
    }
    if (tid < 16) *reinterpret_cast<uint4 *>(smem + Geo::ZERO_OFF + (tid << 4)) = make_uint4(0, 0, 0, 0);
    // the head conv weights are fetched here, behind the loads the prologue waits for anyway (the first version fetched
    // them after the last layer: one more exposed round trip and barrier per workgroup)
    if (head_out && tid < 3 * 128 / 4)
        reinterpret_cast<float4 *>(smem + Geo::HEADW_OFF)[tid] = reinterpret_cast<const float4 *>(head_w)[tid];
    // first-layer weights: requested before the wait below so that their latency overlaps the planes / ring prologue
    bf16x8 wf[9][CV_CT];
    if (planes != nullptr) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int j = 0; j < CV_CT; ++j)
                wf[t][j] = *reinterpret_cast<const bf16x8 *>(w0 + ((size_t)((t * 2 + (lane >> 5)) * 128 + (wave & 1) * 64 + j * 32 + (lane & 31)) << 3));
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // per lane and owned tile: the own cell (row | key << 9 | live << 13), its 32 bytes of input planes, and for each of the nine
    // taps the neighbour's row (360 = the zero row when it is off the board), 9 bits each, three taps per register.  The neighbour's
    // KEY needs no table: key(p, y + dy, x + dx) is the own key with bit 3 flipped for dy = +-1 and dx + dy added to its low three
    // bits — for an off-board neighbour too, which reads the zero row in the slot its (virtual) cell would have used, so every
    // ds_read_b128 group stays on 16 distinct slots (a padding lane's key is its lane number)
    // Which lane owns which GEMM row of a tile is free (the lane's addresses come from its own tables) and follows the LDS: a
    // ds_read_b128 is served in the NON-contiguous lane groups {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} (+ 32 for the upper
    // half-wave; MI355X_MICROARCH.md, LDS), so those lanes get the 16 consecutive GEMM rows — two board rows of eight cells —
    // whose neighbours' keys are distinct (with rows in lane order the groups mix four board rows: measured 31 % of the LDS
    // cycles in bank conflicts instead of 8 %)
    const int m31 = l31 < 4 ? l31 : l31 < 12 ? l31 + 12 : l31 < 16 ? l31 - 8 : l31 < 20 ? l31 + 8 : l31 < 28 ? l31 - 12 : l31;
    int own[CV_RT], natb[CV_RT], nb[CV_RT][3];
#pragma unroll
    for (int i = 0; i < CV_RT; ++i) {
        const int k = 32 * (wr + 4 * i) + m31 - 24;       // LDS row; k < 0: one of the 24 padding rows
        int p = 0, y = 0, x = 0;
        if (k >= 200 || (k >= 104 && k < 168)) { const int j = k >= 200 ? k - 136 : k - 104; p = j / 56; const int r = j - p * 56; y = (r >> 3) + 1; x = (r & 7) + 1; }
        else if (k >= 168) { p = (k - 168) >> 3; y = ((k - 168) & 7) + 1; x = 9; }
        else if (k >= 72) { p = (k - 72) >> 3; y = 8; x = ((k - 72) & 7) + 1; }
        else if (k >= 40) { p = (k - 40) >> 3; y = ((k - 40) & 7) + 1; x = 0; }
        else if (k >= 8) { p = (k - 8) >> 3; x = (k - 8) & 7; }
        else if (k >= 0) { p = k >> 1; x = 8 + (k & 1); }
        const bool live = k >= 0;
        own[i] = live ? (k | (key_of(p, y, x) << 9) | (1 << 13)) : ((m31 & 15) << 9);
        natb[i] = (p * 90 + y * 10 + x) * 32;
#pragma unroll
        for (int q = 0; q < 3; ++q) nb[i][q] = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            const bool valid = live && yy >= 0 && yy < 9 && xx >= 0 && xx < 10;
            nb[i][t / 3] |= (valid ? row_of(p, yy, xx) : Geo::ROWS) << (9 * (t % 3));
        }
    }
    static_assert(Geo::ZERO_OFF == Geo::ROWS * CV_ROWB, "the zero row is row ROWS");
    auto nb_row = [&](int i, int tap) -> int {   // tap is a compile-time constant wherever the product path calls this
        const int sel = tap / 3;
        int r = nb[i][0];
        r = sel == 1 ? nb[i][1] : r; r = sel >= 2 ? nb[i][2] : r;
        return (r >> (9 * (tap - 3 * sel))) & 511;
    };
    // everything derived from nb / own is loop-invariant over the layers: without an opaque copy per layer hipcc hoists the 54 tap
    // addresses and keys out of the layer loop and spills (the same trick as refresh_rb below)
    auto refresh_nb = [&]() {
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) {
            asm volatile("" : "+v"(own[i]));
#pragma unroll
            for (int q = 0; q < 3; ++q) asm volatile("" : "+v"(nb[i][q]));
        }
    };
    auto tap_addr = [&](int tap_, int (&ab)[CV_RT], int (&key)[CV_RT]) {
        const int tap = tap_ < 9 ? tap_ : 8;   // the prefetch behind the last tap reads something harmless
        const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) {
            const int k4 = (own[i] >> 9) & 15;
            ab[i] = nb_row(i, tap) * CV_ROWB;
            key[i] = ((((k4 >> 3) ^ dy) & 1) << 3 | ((k4 + dx + dy) & 7)) ^ khalf;
        }
    };
    const int vb0 = Geo::W_OFF + khalf * 2048 + ((wc * 64 + l31) << 4);
    int keep;

    // the cells / channel quads this lane owns in the accumulator layout
    // 24 swizzled addresses per lane: recomputed from an opaque copy of the row offset wherever they are needed
    // (hoisted out of the layer loop they are only spilled to scratch)
    int rb[CV_RT];
    auto refresh_rb = [&]() {
#pragma unroll
        for (int i = 0; i < CV_RT; ++i) {
            rb[i] = own[i];
            asm volatile("" : "+v"(rb[i]));
        }
    };
    auto cell_ptr = [&](int i, int j, int q, bool &live) -> uint2 * {
        live = (rb[i] >> 13) & 1;
        const int n0 = wc * 64 + j * 32 + 8 * q + 4 * khalf;
        return reinterpret_cast<uint2 *>(smem + (rb[i] & 511) * CV_ROWB + (((n0 >> 3) ^ ((rb[i] >> 9) & 15)) << 4) + ((n0 & 4) << 1));
    };
    // acc = bias (+ x): the residual is folded into the initialisation of a block's second conv
    uint2 xreg[CV_RT][CV_CT][4];   // block input x at this lane's accumulator positions (packed bf16)
    auto init_acc = [&](f32x16 (&acc)[CV_RT][CV_CT], const float *bl, bool add_x) {
#pragma unroll
        for (int j = 0; j < CV_CT; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 bq = *reinterpret_cast<const float4 *>(bl + wc * 64 + j * 32 + 8 * q + 4 * khalf);
#pragma unroll
                for (int i = 0; i < CV_RT; ++i) {
                    float a0 = bq.x, a1 = bq.y, a2 = bq.z, a3 = bq.w;
                    if (add_x) {
                        const uint2 x = xreg[i][j][q];
                        const f32x2 xl = unpack_pair<F16>(x.x), xh = unpack_pair<F16>(x.y);
                        a0 += xl[0]; a1 += xl[1]; a2 += xh[0]; a3 += xh[1];
                    }
                    acc[i][j][4 * q + 0] = a0; acc[i][j][4 * q + 1] = a1; acc[i][j][4 * q + 2] = a2; acc[i][j][4 * q + 3] = a3;
                }
            }
    };
    // ReLU -> bf16 -> U, in place (callers put a barrier in front: every wave must be done reading U)
    auto store_layer = [&](f32x16 (&acc)[CV_RT][CV_CT]) {
#pragma unroll
        for (int i = 0; i < CV_RT; ++i)
#pragma unroll
            for (int j = 0; j < CV_CT; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    bool live;
                    uint2 *cell = cell_ptr(i, j, q, live);
                    // ReLU after the rounding, as a packed signed-16-bit max with 0: a bf16 / fp16 is negative exactly when
                    // its bit pattern is a negative int16 and RNE never changes the sign, so the result is the same
                    // as relu-then-round at a quarter of the VALU work (no v_max_f32 + canonicalize per element)
                    const s16x2 z = {0, 0};
                    s16x2 rl = __builtin_elementwise_max(
                        __builtin_bit_cast(s16x2, pack_pair<F16>(f32x2{acc[i][j][4 * q + 0], acc[i][j][4 * q + 1]})), z);
                    s16x2 rh = __builtin_elementwise_max(
                        __builtin_bit_cast(s16x2, pack_pair<F16>(f32x2{acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]})), z);
                    if constexpr (F16) {   // fp16 only: +inf (0x7C00) and NaN patterns are the int16 values above 0x7BFF = 65504:
                        const s16x2 top = {0x7BFF, 0x7BFF};   // an activation beyond the half range saturates instead of
                        rl = __builtin_elementwise_min(rl, top);   // putting inf / NaN into every later layer and the priors
                        rh = __builtin_elementwise_min(rh, top);
                    }
                    if (live) *cell = make_uint2(__builtin_bit_cast(uint32_t, rl), __builtin_bit_cast(uint32_t, rh));
                }
    };

    if (planes != nullptr) {   // first layer: conv3x3(14 -> 128) + BN + ReLU, one k-step per tap
        f32x16 acc[CV_RT][CV_CT];
        init_acc(acc, b0, false);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int shift = (t / 3 - 1) * 10 + (t % 3 - 1);
            bf16x8 af[CV_RT];
#pragma unroll
            for (int i = 0; i < CV_RT; ++i) {
                const int a = nb_row(i, t) != Geo::ROWS ? Geo::PLANES_OFF + (natb[i] + shift * 32) : Geo::ZERO_OFF;
                af[i] = *reinterpret_cast<const bf16x8 *>(smem + a + khalf * 16);
            }
#pragma unroll
            for (int i = 0; i < CV_RT; ++i)
#pragma unroll
                for (int j = 0; j < CV_CT; ++j)
                    acc[i][j] = mfma_32x32x16<F16>(wf[t][j], af[i], acc[i][j]);
        }
        refresh_rb();
        store_layer(acc);    // U is not read by the first conv: no barrier needed in front
        __syncthreads();
    }

#define T8_OPERANDS(NAB, NKEY)                                                                                   \
            : [c00] "+v"(acc[0][0]), [c01] "+v"(acc[0][1]), [c10] "+v"(acc[1][0]), [c11] "+v"(acc[1][1]),          \
              [c20] "+v"(acc[2][0]), [c21] "+v"(acc[2][1]),                                                        \
              [f0a0] "+v"(f0.a[0]), [f0a1] "+v"(f0.a[1]), [f0a2] "+v"(f0.a[2]), [f0b0] "+v"(f0.b[0]), [f0b1] "+v"(f0.b[1]), \
              [f1a0] "=&v"(f1.a[0]), [f1a1] "=&v"(f1.a[1]), [f1a2] "=&v"(f1.a[2]), [f1b0] "=&v"(f1.b[0]), [f1b1] "=&v"(f1.b[1]), \
              [t0] "=&v"(t0), [t1] "=&v"(t1), [t2] "=&v"(t2), [keep] "=&s"(keep)                                     \
            : [ab0] "v"(ab[0]), [ab1] "v"(ab[1]), [ab2] "v"(ab[2]), [key0] "v"(key[0]), [key1] "v"(key[1]),          \
              [key2] "v"(key[2]), [nab0] "v"(NAB[0]), [nab1] "v"(NAB[1]), [nab2] "v"(NAB[2]), [nkey0] "v"(NKEY[0]),   \
              [nkey1] "v"(NKEY[1]), [nkey2] "v"(NKEY[2]), [vb] "v"(vb), [vbn] "v"(vbn), [voff0] "v"(voff0),          \
              [voff1] "v"(voff1), [sbase] "s"(sbase), [ldst] "s"(ldst)
#define T8_SLAB(ASMSTR, NAB, NKEY)    /* the bodies' s_add_u32 (M0 stepping) writes SCC */                        \
        asm volatile(ASMSTR T8_OPERANDS(NAB, NKEY) : "memory", "scc")
#define T8_SLABV(ASMSTR, NAB, NKEY)   /* the same operands + the wave-uniform skip mask; clobbers VCC */          \
        asm volatile(ASMSTR T8_OPERANDS(NAB, NKEY), [skipm] "s"(skipm) : "memory", "vcc", "scc")
#define T8_SLAB_ARGS() TRUNK_SLAB_ARGS(reinterpret_cast<const unsigned char *>(wpk), )
#define T8_RUNV(BF, HF, NAB, NKEY)                                                                              \
        {                                                                                                       \
            T8_SLAB_ARGS()                                                                                      \
            if constexpr (F16) { T8_SLABV(HF, NAB, NKEY); } else { T8_SLABV(BF, NAB, NKEY); }                   \
            ++g;                                                                                                \
        }
#define T8_RUN(BF, HF, NAB, NKEY)                                                                               \
        {                                                                                                       \
            T8_SLAB_ARGS()                                                                                      \
            if constexpr (F16) { T8_SLAB(HF, NAB, NKEY); } else { T8_SLAB(BF, NAB, NKEY); }                     \
            ++g;                                                                                                \
        }

    int g = 0;
    // which of the wave's first two tiles (slot 0: tile wr, slot 1: tile wr + 4) is off the board for a tap: two bits per tap.
    // Groups 0, 1: the rank-0 tiles (taps 0..2); group 2: the file-0 tile (taps 0, 3, 6) and the file-9 tile (slot 1: taps 2, 5, 8);
    // group 3: the rank-8 tile (taps 6..8).  The slab bodies branch around those tiles' MFMAs (adding 0 * w is exact: the outputs
    // are bit-identical); per SIMD the skipped MFMAs balance in taps 0, 1, 2, 6 and 8 (1/6 of the slab's) — 5/54 of a layer's.
    const int skiptab = __builtin_amdgcn_readfirstlane(wr < 2 ? 0x15 : (wr == 2 ? 0x21861 : 0x15000));
#pragma unroll 1
    for (int layer = 0; layer < nlayers; ++layer) {
        f32x16 acc[CV_RT][CV_CT];
        CZ_T8_STAMP(0);
        refresh_nb();
        refresh_rb();
        if (!(layer & 1)) {   // first conv of a block: remember x, start from the bias
#pragma unroll
            for (int i = 0; i < CV_RT; ++i)
#pragma unroll
                for (int j = 0; j < CV_CT; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) { bool live; xreg[i][j][q] = *cell_ptr(i, j, q, live); }
            init_acc(acc, bias + layer * 128, false);
        } else {
            init_acc(acc, bias + layer * 128, true);
        }
        int ab[CV_RT], key[CV_RT], nab[CV_RT], nkey[CV_RT], t0, t1, t2;
        TwFrag f0, f1;
        tap_addr(0, ab, key);
        {
            const int vb = vb0 + (((unsigned)g & 3u) << Geo::SLAB_SHIFT);
            TW_LOADSET(0, 0, 512, f0, ab, key, vb);   // waited for by the first k-step itself
        }
        CZ_T8_STAMP(1);
#if defined(CZ_T8_SKIPTEST)   // measurement only (tools/experiments/tower_skip_ubench.hip; never defined in the library): the first
        // CZ_T8_SKIPTEST taps of every layer run a slab body WITHOUT the MFMAs of the wave's third cell tile — wrong results;
        // what issuing 1/9 .. 1/3 fewer MFMAs buys in wall time under the power governor (zero-work removal).  A
        // loop of its own: the two slab bodies under one branch made hipcc copy the accumulators at the join
        int tap = 0;
#pragma unroll 1
        for (; tap < CZ_T8_SKIPTEST; ++tap) {
            T8_RUN(TW8_SKIP_ASM_H0, TW8F_SKIP_ASM_H0, ab, key)
            tap_addr(tap + 1, nab, nkey);
            T8_RUN(TW8_SKIP_ASM_H1, TW8F_SKIP_ASM_H1, nab, nkey)
#pragma unroll
            for (int i = 0; i < CV_RT; ++i) { ab[i] = nab[i]; key[i] = nkey[i]; }
        }
#pragma unroll 1
        for (; tap < 9; ++tap) {
            T8_RUN(TW8_SLAB_ASM_H0, TW8F_SLAB_ASM_H0, ab, key)
            tap_addr(tap + 1, nab, nkey);
            T8_RUN(TW8_SLAB_ASM_H1, TW8F_SLAB_ASM_H1, nab, nkey)
#pragma unroll
            for (int i = 0; i < CV_RT; ++i) { ab[i] = nab[i]; key[i] = nkey[i]; }
        }
#else
        // the nine taps unrolled: the neighbour fields come out of their registers with constant shifts, the skip bits of a tap are
        // one s_bfe.  Two 16 KB slabs per tap; tap 4 (the centre) has nothing to skip and runs the plain bodies
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap == 4) {
                T8_RUN(TW8_SLAB_ASM_H0, TW8F_SLAB_ASM_H0, ab, key)
                tap_addr(tap + 1, nab, nkey);
                T8_RUN(TW8_SLAB_ASM_H1, TW8F_SLAB_ASM_H1, nab, nkey)
            } else {
                const int skipm = __builtin_amdgcn_readfirstlane((skiptab >> (2 * tap)) & 3);
                T8_RUNV(TW8_SKIPG_ASM_H0, TW8F_SKIPG_ASM_H0, ab, key)
                tap_addr(tap + 1, nab, nkey);
                T8_RUNV(TW8_SKIPG_ASM_H1, TW8F_SKIPG_ASM_H1, nab, nkey)
            }
#pragma unroll
            for (int i = 0; i < CV_RT; ++i) { ab[i] = nab[i]; key[i] = nkey[i]; }
#if defined(CZ_T8_TRACE) && CZ_T8_TRACE >= 2
            CZ_T8_STAMP(4 + tap);
#endif
        }
#endif
        // the last k-step prefetched garbage for a non-existent next slab; drain it, let the MFMAs retire, and make
        // sure every wave is done reading U before anyone overwrites it in place
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
        CZ_T8_STAMP(2);
        __syncthreads();
#if defined(CZ_T8_TRACE)
        CZ_T8_STAMP(13);   // through the barrier: 13 - 2 = this wave's wait for the slowest wave of the workgroup
#endif
        refresh_rb();
        store_layer(acc);
        __syncthreads();
        CZ_T8_STAMP(3);
    }
    if (clk && tid == 0) {   // the layers are done; the epilogue below (trunk dump / head convs) is ~1 % of the workgroup's life
        clk[blockIdx.x * 4 + 0] = clk_c0; clk[blockIdx.x * 4 + 1] = __builtin_readcyclecounter();
        clk[blockIdx.x * 4 + 2] = clk_r0; clk[blockIdx.x * 4 + 3] = __builtin_amdgcn_s_memrealtime();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (out) {
        uint4 *go = reinterpret_cast<uint4 *>(out + (size_t)pos0 * 90 * 128);
        for (int idx = tid; idx < nrows * 16; idx += Geo::THREADS) {
            const int r = idx >> 4, c = idx & 15;
            go[idx] = *reinterpret_cast<const uint4 *>(smem + lds_of_natural(r, c));
        }
    }
    if (head_out) {
        const float *hw = reinterpret_cast<const float *>(smem + Geo::HEADW_OFF);   // staged at the prologue
        // one thread per board cell, all three head channels: the cell's 256-byte row is read and unpacked once (the first
        // version gave every (cell, channel) pair its own thread: three reads and unpacks of every row, 5 us per workgroup).
        // The summation order per (cell, channel) is unchanged — chunks in a fixed order, eight products left to right —
        // so the outputs are bit-identical to the earlier kernel and do not depend on the row's position in the batch.
        for (int r = tid; r < nrows; r += Geo::THREADS) {
            const int l0 = lds_of_natural(r, 0), rowoff = l0 & ~(CV_ROWB - 1), key = (l0 >> 4) & 15;   // chunk 0 sits in slot key
            float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
#pragma unroll 4
            for (int c = 0; c < 16; ++c) {
                const int p = c ^ key;
                const uint4 v = *reinterpret_cast<const uint4 *>(smem + rowoff + (p << 4));
                const f32x2 e0 = unpack_pair<F16>(v.x), e1 = unpack_pair<F16>(v.y), e2 = unpack_pair<F16>(v.z), e3 = unpack_pair<F16>(v.w);
                const float *w0 = hw + c * 8, *w1 = hw + 128 + c * 8, *w2 = hw + 256 + c * 8;
                acc0 += e0[0] * w0[0] + e0[1] * w0[1] + e1[0] * w0[2] + e1[1] * w0[3]
                      + e2[0] * w0[4] + e2[1] * w0[5] + e3[0] * w0[6] + e3[1] * w0[7];
                acc1 += e0[0] * w1[0] + e0[1] * w1[1] + e1[0] * w1[2] + e1[1] * w1[3]
                      + e2[0] * w1[4] + e2[1] * w1[5] + e3[0] * w1[6] + e3[1] * w1[7];
                acc2 += e0[0] * w2[0] + e0[1] * w2[1] + e1[0] * w2[2] + e1[1] * w2[3]
                      + e2[0] * w2[4] + e2[1] * w2[5] + e3[0] * w2[6] + e3[1] * w2[7];
            }
            float *o = head_out + ((size_t)pos0 * 90 + r) * 3;
            o[0] = fmaxf(acc0 + head_b[0], 0.f);
            o[1] = fmaxf(acc1 + head_b[1], 0.f);
            o[2] = fmaxf(acc2 + head_b[2], 0.f);
        }
    }
}
#undef T8_OPERANDS
#undef T8_SLAB
#undef T8_SLABV
#undef T8_SLAB_ARGS
#undef T8_RUN
#undef T8_RUNV


#undef TW_LOADSET
#undef CV_LD
#undef CV_ST
}  // namespace czconv
