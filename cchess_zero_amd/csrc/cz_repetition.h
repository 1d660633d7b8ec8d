// cz_repetition.h — the repetition rule of include/cchess_hip.h (cz_repetition), evaluated by one wave64 on one game's history.
// Used by the stand-alone call (cz_repetition.hip: the caller's own record) and by the match (cz_match.hip: the slot's ring of
// 64 positions).  No reference function: the reference's games have no repetition rule.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/cchess_hip.h"

// Position i of the history is at keys[i & imask] / in_check[i & imask]: imask = 63 for the match's ring, 0x7fffffff for a
// caller's record.  n: the current position, with key key_n, check flag chk_n and side to move side_n (the earlier sides follow
// by parity); w <= n: how many earlier positions count; fold >= 2.
// Lane l of a chunk looks at position n - 1 - (base + l): the lanes with the current key are the earlier occurrences, most
// recent first, and the (fold - 1)-th of them is `first` = j; the cycle is j + 1 .. n.  Side X checked perpetually when every
// position of the cycle with side 1 - X to move (at least one) is a check.  -> CZ_REP_*, wave-uniform; first = -1 without a verdict.
__device__ __forceinline__ int wave_repetition(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check, int imask,
                                               int n, int w, uint64_t key_n, bool chk_n, int side_n, int fold, int lane, int &first) {
    first = -1;
    int need = fold - 1;
    // quiet[s]: a position of the cycle with side s to move is no check; seen[s]: the cycle has a position with side s to move
    bool quiet[2] = {false, false}, seen[2] = {false, false};
    seen[side_n & 1] = true;
    quiet[side_n & 1] = !chk_n;
    for (int base = 0; base < w; base += 64) {   // the match never takes a second chunk (w <= 63)
        const int l = base + lane, i = n - 1 - l;
        const bool valid = l < w;
        const uint64_t k = valid ? keys[i & imask] : 0ull;
        const bool c = valid && in_check[i & imask] != 0;
        unsigned long long eq = __ballot(valid && k == key_n);
        const int cnt = __popcll(eq);
        int upto = 64;                           // the lanes below it are inside the cycle
        if (cnt >= need) {
            for (int s = 1; s < need; ++s) eq &= eq - 1ull;   // drop the more recent occurrences: fold <= 8
            upto = __ffsll((long long)eq) - 1;
            first = n - 1 - (base + upto);
        }
        const bool in = valid && lane < upto;
        const int stm = (side_n ^ (l + 1)) & 1;  // position i is l + 1 plies before n
        if (__ballot(in && stm == 0)) seen[0] = true;
        if (__ballot(in && stm == 1)) seen[1] = true;
        if (__ballot(in && stm == 0 && !c)) quiet[0] = true;
        if (__ballot(in && stm == 1 && !c)) quiet[1] = true;
        if (first >= 0) break;
        need -= cnt;
    }
    if (first < 0) return CZ_REP_NONE;
    const bool red = seen[1] && !quiet[1], black = seen[0] && !quiet[0];   // red checked with every move / black did
    return red == black ? CZ_REP_DRAW : (red ? CZ_REP_RED_LOSES : CZ_REP_BLACK_LOSES);
}
