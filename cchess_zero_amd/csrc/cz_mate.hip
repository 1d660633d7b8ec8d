// cz_mate.hip — cz_mate_backup: the backward pass of the forced-mate search (Rules.mate).  The children of parent g are the
// range [offsets[g], offsets[g + 1]) of child_dist / child_label / child_pv, as cz_successors lays them out; a child's dist is
// the number of plies until the defender is mated, CZ_MATE_NONE when that is not proven.  An attacker's parent (mode 0, OR)
// takes 1 + the minimum over its proven children, a defender's (mode 1, AND) 1 + the maximum when every child is proven and 0
// when it has no child; the FIRST child in list order that attains the value gives the line: its label, then its own line.
// ONE LANE PER PARENT.  The pass reads 2 bytes per child (4 + 2 W more for the one best child of a parent) behind a
// cz_successors that wrote 106 bytes for each of them, so its traffic is a few per cent of the slice's and nothing is staged:
// a lane walks its own ~40 consecutive halfwords, neighbouring lanes' ranges are neighbours in memory, and every 64-byte line
// that one step of the wave touches serves the following steps from the cache.  A wave per 64 parents that strides over the
// group's children would coalesce these loads and pay a segmented reduction with first-index ties for it; the AND mode's early
// exit (one unproven child decides the parent) is per lane here.  Offsets are clamped into [0, total] as in cz_successors:
// whatever they hold, no access leaves the arrays.
#include "cz_internal.h"

namespace {

__global__ __launch_bounds__(256) void k_mate_backup(const int32_t *__restrict__ offsets, int G, int total, const int16_t *__restrict__ child_dist,
                                                     const uint16_t *__restrict__ child_label, const uint16_t *__restrict__ child_pv, int W,
                                                     int mode, int16_t *__restrict__ out_dist, uint16_t *__restrict__ out_pv) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int c0 = min(max(offsets[g], 0), total), c1 = min(max(offsets[g + 1], c0), total);
    int best = -1, bd = mode ? -1 : CZ_MATE_NONE;
    bool open = false;   // mode 1: a child that is not proven
    for (int c = c0; c < c1; ++c) {
        const int d = child_dist[c];
        const bool proven = (unsigned)d < (unsigned)CZ_MATE_NONE;
        if (mode) {
            if (!proven) { open = true; break; }
            if (d > bd) { bd = d; best = c; }
        } else if (proven && d < bd) {
            bd = d; best = c;
        }
    }
    int dist = mode ? (open ? CZ_MATE_NONE : bd + 1) : (best >= 0 ? bd + 1 : CZ_MATE_NONE);   // mode 1 without children: bd + 1 = 0
    if (dist == CZ_MATE_NONE || dist == 0) best = -1;
    out_dist[g] = (int16_t)dist;
    uint16_t *const row = out_pv + (size_t)g * (W + 1);
    row[0] = best >= 0 ? child_label[best] : (uint16_t)0xFFFF;
    for (int k = 0; k < W; ++k) row[1 + k] = best >= 0 ? child_pv[(size_t)best * W + k] : (uint16_t)0xFFFF;
}

}  // namespace

int cz_mate_backup(cz_ctx *c, const int32_t *offsets, int G, int total, const int16_t *child_dist, const uint16_t *child_label,
                   const uint16_t *child_pv, int W, int mode, int16_t *out_dist, uint16_t *out_pv) {
    CZ_REQUIRE(c && G >= 0 && total >= 0, "cz_mate_backup: null ctx / negative G or total");
    CZ_REQUIRE(W >= 0 && W <= CZ_MATE_MAX_LINE, "cz_mate_backup: W is 0 .. CZ_MATE_MAX_LINE");
    CZ_REQUIRE(mode == 0 || mode == 1, "cz_mate_backup: mode is 0 (attacker, OR) or 1 (defender, AND)");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(offsets && out_dist && out_pv, "cz_mate_backup: offsets, out_dist, out_pv required");
    CZ_REQUIRE(total == 0 || (child_dist && child_label && (W == 0 || child_pv)), "cz_mate_backup: child_dist, child_label, child_pv (W > 0) required");
    hipLaunchKernelGGL(k_mate_backup, dim3((G + 255) / 256), dim3(256), 0, c->stream, offsets, G, total, child_dist, child_label, child_pv, W, mode,
                       out_dist, out_pv);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
