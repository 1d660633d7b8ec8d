// cz_repetition.hip — cz_repetition: the repetition rule (cz_repetition.h) on G game records that the caller keeps, and
// cz_repetition_chase: the same with the chase verdict behind it (wave_repetition_chase, on the records of cz_threats).  One
// wave64 per game, walking its games with a stride; a history of more than 64 earlier positions is read in chunks of 64, most
// recent first, and the walk stops at the chunk that holds the (fold - 1)-th occurrence.  A byte kernel: 9 bytes per position
// read (41 with the chase records).
#include "cz_internal.h"
#include "cz_repetition.h"

namespace {

// CHASE = false: chase and cause are not looked at (cz_repetition passes NULL)
template <bool CHASE>
__global__ __launch_bounds__(64) void k_repetition(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check,
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
            if constexpr (CHASE) {
                const uint64_t *r = chase + (size_t)g * stride * 4;
                const uint64_t rec_n[4] = {r[(size_t)n * 4], r[(size_t)n * 4 + 1], r[(size_t)n * 4 + 2], r[(size_t)n * 4 + 3]};
                v = wave_repetition_chase(k, c, r, 0x7fffffff, n, w, k[n], c[n] != 0, rec_n, side[g] ? 1 : 0, fold, lane, j, why);
            } else {
                v = wave_repetition(k, c, 0x7fffffff, n, w, k[n], c[n] != 0, side[g] ? 1 : 0, fold, lane, j);
            }
        }
        if (lane == 0) {
            verdict[g] = (uint8_t)v;
            if (first) first[g] = j;
            if (CHASE && cause) cause[g] = (uint8_t)why;
        }
    }
}

}  // namespace

int cz_repetition(cz_ctx *c, const uint64_t *keys, const uint8_t *in_check, int stride, const int32_t *len, const int32_t *window,
                  const uint8_t *side, int G, int fold, uint8_t *verdict, int32_t *first) {
    CZ_REQUIRE(c && G >= 0, "cz_repetition: null ctx / negative G");
    CZ_REQUIRE(fold >= 2 && fold <= 8, "cz_repetition: 2 <= fold <= 8");
    CZ_REQUIRE(stride >= 1, "cz_repetition: stride >= 1");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(keys && in_check && len && side && verdict, "cz_repetition: keys, in_check, len, side, verdict required");
    hipLaunchKernelGGL(k_repetition<false>, dim3(G < 65536 ? G : 65536), dim3(64), 0, c->stream, keys, in_check, (const uint64_t *)nullptr, stride,
                       len, window, side, G, fold, verdict, first, (uint8_t *)nullptr);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_repetition_chase(cz_ctx *c, const uint64_t *keys, const uint8_t *in_check, const uint64_t *chase, int stride, const int32_t *len,
                        const int32_t *window, const uint8_t *side, int G, int fold, uint8_t *verdict, int32_t *first, uint8_t *cause) {
    CZ_REQUIRE(c && G >= 0, "cz_repetition_chase: null ctx / negative G");
    CZ_REQUIRE(fold >= 2 && fold <= 8, "cz_repetition_chase: 2 <= fold <= 8");
    CZ_REQUIRE(stride >= 1, "cz_repetition_chase: stride >= 1");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(keys && in_check && chase && len && side && verdict, "cz_repetition_chase: keys, in_check, chase, len, side, verdict required");
    hipLaunchKernelGGL(k_repetition<true>, dim3(G < 65536 ? G : 65536), dim3(64), 0, c->stream, keys, in_check, chase, stride, len, window, side,
                       G, fold, verdict, first, cause);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
