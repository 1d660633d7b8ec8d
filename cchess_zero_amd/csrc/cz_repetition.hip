// cz_repetition.hip — cz_repetition: the repetition rule (cz_repetition.h) on G game records that the caller keeps.  One wave64
// per game, walking its games with a stride; a history of more than 64 earlier positions is read in chunks of 64, most recent
// first, and the walk stops at the chunk that holds the (fold - 1)-th occurrence.  A byte kernel: 9 bytes per position read.
#include "cz_internal.h"
#include "cz_repetition.h"

namespace {

__global__ __launch_bounds__(64) void k_repetition(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check, int stride,
                                                   const int32_t *__restrict__ len, const int32_t *__restrict__ window,
                                                   const uint8_t *__restrict__ side, int G, int fold, uint8_t *__restrict__ verdict,
                                                   int32_t *__restrict__ first) {
    const int lane = threadIdx.x;
    for (int g = blockIdx.x; g < G; g += gridDim.x) {
        const int L = len[g];
        int v = CZ_REP_NONE, j = -1;
        if (L >= 1 && L <= stride) {   // a length outside the record answers "no verdict": nothing behind the row is read
            const int n = L - 1;
            const int w = window ? max(0, min(window[g], n)) : n;
            const uint64_t *k = keys + (size_t)g * stride;
            const uint8_t *c = in_check + (size_t)g * stride;
            v = wave_repetition(k, c, 0x7fffffff, n, w, k[n], c[n] != 0, side[g] ? 1 : 0, fold, lane, j);
        }
        if (lane == 0) {
            verdict[g] = (uint8_t)v;
            if (first) first[g] = j;
        }
    }
}

}  // namespace

int czk_repetition(cz_ctx *c, const uint64_t *keys, const uint8_t *in_check, int stride, const int32_t *len, const int32_t *window,
                   const uint8_t *side, int G, int fold, uint8_t *verdict, int32_t *first) {
    if (G == 0) return CZ_OK;
    hipLaunchKernelGGL(k_repetition, dim3(G < 65536 ? G : 65536), dim3(64), 0, c->stream, keys, in_check, stride, len, window, side, G, fold,
                       verdict, first);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
