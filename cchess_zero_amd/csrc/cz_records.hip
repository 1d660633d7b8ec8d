// cz_records.hip — packed self-play records -> the training tuples (planes, pi, z) on the device, with the board's left-right
// mirror as an argument (cz_records_expand).  The host statement is selfplay.to_dense on records.mirror_records.
//
// One wave per record, CZR_WAVES records per workgroup.  The mirror acts on the BOARD (cell (r, f) is read from (r, 8 - f)) and on
// the LABELS (CzHostTables::mirror), before try_flip / unflip and the plane encoding: the planes are read with the reference's
// 9-stride (quirk Q1), so a flip of the plane tensor is not a board mirror.  A mirrored record keeps its children in the order
// they were generated for the unmirrored board; nothing here depends on that order.
//
// Every output element is written exactly once: a record's pi row is built in the wave's own LDS row (zeroed, scattered into,
// then streamed out), never zero-filled and scattered in global memory.  The waves of a workgroup share nothing, so the only
// fences are the wave's own (CZF_WAVE_FENCE) and a wave past the last record simply leaves.
#include "cz_internal.h"
#include "cz_posframe.h"

#define CZR_WAVES 4                                  /* records per workgroup (records.RECORDS_PER_WORKGROUP) */
#define CZR_ROW ((CZ_NLABELS + 3) / 4 * 4)           /* floats of a wave's LDS row: 2086 rounded up so that every row is 16-byte aligned */

namespace {

__global__ __launch_bounds__(64 * CZR_WAVES) void k_records_expand(const uint8_t *__restrict__ records, int n, const uint8_t *__restrict__ mirror,
                                                                   double inv_temp, const int16_t *__restrict__ unflip,
                                                                   const int16_t *__restrict__ mirror_tab, float *__restrict__ planes,
                                                                   float *__restrict__ pi, float *__restrict__ z) {
    __shared__ __attribute__((aligned(16))) float rows[CZR_WAVES][CZR_ROW];
    __shared__ __attribute__((aligned(16))) uint8_t boards[CZR_WAVES][CZD_BOARD_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *row = rows[wave];
    uint8_t *b = boards[wave];
    const long long ngroups = ((long long)n + CZR_WAVES - 1) / CZR_WAVES;
    for (long long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const long long i = grp * CZR_WAVES + wave;
        if (i >= n) return;   // no barrier below: the other waves go on
        const uint8_t *__restrict__ r = records + (size_t)i * CZ_REC_BYTES;
        const int side = r[CZ_REC_SIDE] ? 1 : 0;
        const int count = min((int)r[CZ_REC_COUNT], CZD_MAXMOVES);
        const bool mir = mirror && mirror[i] != 0;
        CZF_WAVE_FENCE();   // the previous record's board and row have been read
        // the board, cell q from its file mirror when asked for; the padding is zero
        if (lane + 64 < CZD_BOARD_LDS) {
            const int q = lane + 64;
            b[q] = q < CZ_NSQ ? r[mir ? q / 9 * 9 + 8 - q % 9 : q] : (uint8_t)0;
        }
        b[lane] = r[mir ? lane / 9 * 9 + 8 - lane % 9 : lane];
        for (int k = lane; k < CZR_ROW / 4; k += 64) reinterpret_cast<float4 *>(row)[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        // the children at lane and lane + 64: label (mirrored, then rank-flipped for black, main.py:1507-1512) and visit count
        int N[2], lab[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            int l = -1;
            N[h] = 0;
            if (c < count) {
                l = reinterpret_cast<const uint16_t *>(r + CZ_REC_LABELS)[c];
                N[h] = reinterpret_cast<const uint16_t *>(r + CZ_REC_VISITS)[c];
                if (l >= CZ_NLABELS) l = -1;   // not a label: the child has no cell in pi
                if (l >= 0 && mir) l = mirror_tab[l];
                if (l >= 0 && side) l = unflip[l];
                if (l >= CZ_NLABELS) l = -1;
            }
            lab[h] = l;
        }
        double p[2];
        wave_visit_policy(N, count, inv_temp, lane, p);
        CZF_WAVE_FENCE();   // the row is zero, the board is in place
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (lab[h] >= 0) row[lab[h]] = (float)p[h];
        czd_wave_encode_planes<float>(b, side, 1, planes + (size_t)i * (CZ_NSQ * 14), 14, 1.0f, lane);
        if (lane == 0) z[i] = (float)(int8_t)r[CZ_REC_Z];
        CZF_WAVE_FENCE();   // the row is complete
        // a pi row starts at a multiple of 8344 bytes: 8-byte pieces, 512 contiguous bytes per store instruction
        float2 *__restrict__ out = reinterpret_cast<float2 *>(pi + (size_t)i * CZ_NLABELS);
        for (int k = lane; k < CZ_NLABELS / 2; k += 64) out[k] = reinterpret_cast<const float2 *>(row)[k];
    }
}

}  // namespace

int cz_records_expand(cz_ctx *c, const uint8_t *records, int n, const uint8_t *mirror, double temperature, float *planes, float *pi, float *z) {
    CZ_REQUIRE(c && n >= 0, "cz_records_expand: null ctx / negative n");
    CZ_REQUIRE(temperature > 0.0, "cz_records_expand: temperature > 0 required");   // false for a NaN too
    CZ_REQUIRE(planes && pi && z, "cz_records_expand: planes, pi, z required");
    if (n == 0) return CZ_OK;
    CZ_REQUIRE(records, "cz_records_expand: records required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(records) & 3u) == 0 && (reinterpret_cast<uintptr_t>(pi) & 7u) == 0 &&
                   (reinterpret_cast<uintptr_t>(planes) & 3u) == 0 && (reinterpret_cast<uintptr_t>(z) & 3u) == 0,
               "cz_records_expand: records 4-byte, pi 8-byte, planes and z 4-byte aligned");
    static_assert(CZ_NLABELS % 2 == 0 && CZ_REC_BYTES % 4 == 0, "pi rows leave as 8-byte pieces; records keep their 2-byte fields aligned");
    // 33.8 KB of LDS per workgroup of four waves: 4 persistent workgroups per CU
    const int ngroups = (int)(((long long)n + CZR_WAVES - 1) / CZR_WAVES);
    hipLaunchKernelGGL(k_records_expand, dim3(czf_persistent_grid(ngroups, 4)), dim3(64 * CZR_WAVES), 0, c->stream, records, n, mirror,
                       1.0 / temperature, c->tab.unflip, c->tab_mirror, planes, pi, z);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
