// cz_lines.hip — principal variations read from the device trees (cz_search_lines): for every tree, the lines that start at its
// most visited root candidates and follow the most visited child below them.  Read-only on the trees: no atomics, no stores
// into a pool or a tree record; between complete lock-steps, as cz_search_root_stats.
//
// Tie rules, the ones the choosers have (cz_internal.h):
//   candidates   the root's children in generation order, with root_allowed only those whose label has its bit set — the list
//                of wave_root_candidates, as k_match_choose / k_sp_choose get it under rules = 1
//   ranking      more visits first, earlier in generation order first among equals: rank 0 is wave_most_visited's pick, the
//                move cz_search_pick_ready / cz_match_choose play greedily
//   below        the first maximum of N over the children (wave_most_visited); a best child without a visit ends the line
// One wave64 per (tree, line): workgroups of 64, grid G * n_lines.  A line costs one round trip for the root record, one for the
// candidates' labels / visits, and two per level below (the expansion record, then the children's visits).
#include "cz_internal.h"

namespace {

#define CZ_LINES_MAX 128   // n_lines: a root has at most CZD_MAXMOVES children
#define CZ_LINE_LEN_MAX 64 // max_len: a line leaves the wave as one store per output array

__global__ __launch_bounds__(64) void k_lines(CzTrees t, int G, const uint32_t *__restrict__ root_allowed, int n_lines, int max_len,
                                              uint16_t *__restrict__ moves, int32_t *__restrict__ visits, float *__restrict__ q,
                                              uint16_t *__restrict__ len) {
    __shared__ int sN[CZD_MAXMOVES], sI[CZD_MAXMOVES];
    __shared__ int line_n[CZ_LINE_LEN_MAX];
    __shared__ float line_q[CZ_LINE_LEN_MAX];
    __shared__ uint16_t line_mv[CZ_LINE_LEN_MAX];
    const int g = blockIdx.x / n_lines, j = blockIdx.x % n_lines, lane = threadIdx.x;
    if (g >= G) return;
    const TreeView v = view_of(t, g);
    int cb, n;
    root_children(t, g, v, cb, n);
    if (n > CZD_MAXMOVES) n = CZD_MAXMOVES;
    // the candidates' visit counts and child indices, in generation order: each lane's two, and all of them in sN / sI
    int N[2], at[2];
    const int nc = wave_root_candidates(v, cb, n, root_allowed ? root_allowed + (size_t)g * CZ_MASK_WORDS : nullptr, lane, N, at, sN, sI);
    // each lane ranks its two candidates by scanning all of them; the one of rank j starts this line
    int rank[2] = {0, 0};
    const int c0 = lane, c1 = lane + 64;
    const int n0 = N[0], n1 = N[1];
    for (int k = 0; k < nc; ++k) {
        const int nk = sN[k];
        rank[0] += (nk > n0 || (nk == n0 && k < c0)) ? 1 : 0;
        rank[1] += (nk > n1 || (nk == n1 && k < c1)) ? 1 : 0;
    }
    const unsigned long long b0 = __ballot(c0 < nc && rank[0] == j), b1 = __ballot(c1 < nc && rank[1] == j);
    int length = 0;
    if (b0 | b1) {
        const int c = b0 ? __ffsll((long long)b0) - 1 : 64 + __ffsll((long long)b1) - 1;
        int node = cb + sI[c];
        for (;;) {
            if (lane == 0) { line_mv[length] = v.move[node]; line_n[length] = v.N[node]; line_q[length] = v.Q[node]; }
            ++length;
            if (length >= max_len) break;
            const int ccb = v.child_begin[node];
            const int cn = ccb < 0 ? 0 : min((int)v.child_count[node], CZD_MAXMOVES);
            if (cn == 0 || ccb + cn > t.cap) break;   // unexpanded; (a record that points outside the pool ends the line)
            int N[2] = {0, 0};
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (lane + 64 * r < cn) N[r] = v.N[ccb + lane + 64 * r];
            const int bi = wave_most_visited(N, cn, lane);
            const int bn = __shfl(bi < 64 ? N[0] : N[1], bi & 63, 64);
            if (bn <= 0) break;
            node = __builtin_amdgcn_readfirstlane(ccb + bi);
        }
    }
    __syncthreads();
    const size_t line = (size_t)g * n_lines + j;
    if (lane == 0) len[line] = (uint16_t)length;
    if (lane < max_len) {
        const size_t o = line * max_len + lane;
        const bool ok = lane < length;
        if (moves) moves[o] = ok ? line_mv[lane] : (uint16_t)0xFFFF;
        if (visits) visits[o] = ok ? line_n[lane] : 0;
        if (q) q[o] = ok ? line_q[lane] : 0.f;
    }
}

}  // namespace

extern "C" int cz_search_lines(cz_ctx *c, const uint32_t *root_allowed, int n_lines, int max_len, uint16_t *moves, int32_t *visits, float *q,
                               uint16_t *len) {
    CZ_REQUIRE(c && c->G > 0, "cz_search_lines: no search");
    CZ_REQUIRE(n_lines >= 1 && n_lines <= CZ_LINES_MAX, "cz_search_lines: 1 <= n_lines <= 128");
    CZ_REQUIRE(max_len >= 1 && max_len <= CZ_LINE_LEN_MAX, "cz_search_lines: 1 <= max_len <= 64");
    CZ_REQUIRE(len, "cz_search_lines: len is NULL (moves, visits and q may be)");
    hipLaunchKernelGGL(k_lines, dim3((unsigned)c->G * (unsigned)n_lines), dim3(64), 0, c->stream, c->t, c->G, root_allowed, n_lines, max_len,
                       moves, visits, q, len);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
