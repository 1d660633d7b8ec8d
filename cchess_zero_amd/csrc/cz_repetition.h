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
// wave_repetition_ex also says which sides checked perpetually (red / black), which CZ_REP_DRAW folds together: the chase
// verdict below runs only when neither did.
// The _at forms take the history through accessors: key_at(i) / chk_at(i) answer position i < n wherever it is kept (a ring,
// a record, or — cz_repmoves.h — a record with one or two positions behind it that exist in registers only).
template <typename KeyAt, typename ChkAt>
__device__ __forceinline__ int wave_repetition_at(KeyAt key_at, ChkAt chk_at, int n, int w, uint64_t key_n, bool chk_n, int side_n,
                                                  int fold, int lane, int &first, bool &red, bool &black) {
    red = black = false;
    first = -1;
    int need = fold - 1;
    // quiet[s]: a position of the cycle with side s to move is no check; seen[s]: the cycle has a position with side s to move
    bool quiet[2] = {false, false}, seen[2] = {false, false};
    seen[side_n & 1] = true;
    quiet[side_n & 1] = !chk_n;
    for (int base = 0; base < w; base += 64) {   // the match never takes a second chunk (w <= 63)
        const int l = base + lane, i = n - 1 - l;
        const bool valid = l < w;
        const uint64_t k = valid ? key_at(i) : 0ull;
        const bool c = valid && chk_at(i);
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
    red = seen[1] && !quiet[1]; black = seen[0] && !quiet[0];   // red checked with every move / black did
    return red == black ? CZ_REP_DRAW : (red ? CZ_REP_RED_LOSES : CZ_REP_BLACK_LOSES);
}
__device__ __forceinline__ int wave_repetition_ex(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check, int imask,
                                                  int n, int w, uint64_t key_n, bool chk_n, int side_n, int fold, int lane, int &first,
                                                  bool &red, bool &black) {
    return wave_repetition_at([=](int i) { return keys[i & imask]; }, [=](int i) { return in_check[i & imask] != 0; }, n, w, key_n, chk_n,
                              side_n, fold, lane, first, red, black);
}
__device__ __forceinline__ int wave_repetition(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check, int imask,
                                               int n, int w, uint64_t key_n, bool chk_n, int side_n, int fold, int lane, int &first) {
    bool red, black;
    return wave_repetition_ex(keys, in_check, imask, n, w, key_n, chk_n, side_n, fold, lane, first, red, black);
}

// ---- perpetual chase (tests/chase_model.py: verdict).  A position's CHASE RECORD is four 64-bit words (cz_threats): the
// threatened set of the side to move (squares 0 .. 63, 64 .. 89) and that side's squares in the same layout.  Position i's
// record is at chase[(i & imask) * 4]; the current position's is passed in rec_n (the match writes it in the same kernel).
// Side X chases perpetually when one and the same piece of 1 - X is threatened in every position of the cycle j + 1 .. n that
// X's moves led to (1 - X to move; at least one): C = T(first such position); from one such position to the next the victim
// side's squares differ by exactly one "from" and one "to" square (a cycle holds no capture) — a threatened piece on "from" is
// followed to "to", any other difference empties C — and C &= T(next).  -> bit X set: X chases perpetually.
// The walk is serial and wave-uniform: a chunk of 64 positions is loaded one per lane (ascending: lane l holds position
// j + 1 + base + l) and read back lane by lane with __shfl; it stops when neither side has a candidate left.
struct CzChaseSet { uint64_t lo, hi; };
// rec_at(i, r0, r1, r2, r3): the record of position i < n, as the accessors of wave_repetition_at
template <typename RecAt>
__device__ __forceinline__ int wave_chase_at(RecAt rec_at, int n, int j, const uint64_t (&rec_n)[4], int side_n, int lane) {
    // state per victim side v (the side TO MOVE in the positions walked); the loop over v is unrolled: no array is indexed at run time
    CzChaseSet C[2] = {{0ull, 0ull}, {0ull, 0ull}}, prev[2] = {{0ull, 0ull}, {0ull, 0ull}};
    bool started[2] = {false, false}, dead[2] = {false, false};
    const int len = n - j;   // positions j + 1 .. n
    const int v0 = (side_n ^ (len - 1)) & 1;   // the side to move at j + 1 (and at every chunk's lane 0: 64 is even)
    for (int base = 0; base < len; base += 64) {
        if (dead[0] && dead[1]) break;
        const int i = j + 1 + base + lane;
        uint64_t r0 = 0ull, r1 = 0ull, r2 = 0ull, r3 = 0ull;
        if (i < n) {
            rec_at(i, r0, r1, r2, r3);
        } else if (i == n) {
            r0 = rec_n[0]; r1 = rec_n[1]; r2 = rec_n[2]; r3 = rec_n[3];
        }
        const int cnt = min(64, len - base);
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            for (int l = v == v0 ? 0 : 1; l < cnt && !dead[v]; l += 2) {
                const CzChaseSet T = {__shfl(r0, l, 64), __shfl(r1, l, 64)}, own = {__shfl(r2, l, 64), __shfl(r3, l, 64)};
                if (!started[v]) {
                    C[v] = T;
                    started[v] = true;
                } else {
                    const CzChaseSet from = {prev[v].lo & ~own.lo, prev[v].hi & ~own.hi}, to = {own.lo & ~prev[v].lo, own.hi & ~prev[v].hi};
                    const bool one = __popcll(from.lo) + __popcll(from.hi) == 1 && __popcll(to.lo) + __popcll(to.hi) == 1;
                    if (!one) {
                        C[v] = CzChaseSet{0ull, 0ull};
                    } else if ((C[v].lo & from.lo) | (C[v].hi & from.hi)) {
                        C[v].lo = (C[v].lo & ~from.lo) | to.lo;
                        C[v].hi = (C[v].hi & ~from.hi) | to.hi;
                    }
                    C[v].lo &= T.lo;
                    C[v].hi &= T.hi;
                }
                prev[v] = own;
                dead[v] = (C[v].lo | C[v].hi) == 0ull;
            }
        }
    }
    // the chaser of victim v is 1 - v
    return ((started[1] && !dead[1]) ? 1 : 0) | ((started[0] && !dead[0]) ? 2 : 0);
}

__device__ __forceinline__ int wave_chase(const uint64_t *__restrict__ chase, int imask, int n, int j, const uint64_t (&rec_n)[4],
                                          int side_n, int lane) {
    return wave_chase_at([=](int i, uint64_t &r0, uint64_t &r1, uint64_t &r2, uint64_t &r3) {
        const uint64_t *p = chase + (size_t)(i & imask) * 4;
        r0 = p[0]; r1 = p[1]; r2 = p[2]; r3 = p[3];
    }, n, j, rec_n, side_n, lane);
}

// The repetition rule with the chase verdict behind it: wave_repetition's code and first; *cause = CZ_CAUSE_*.  Exactly one
// side checked perpetually: as wave_repetition, cause check (it outranks a chase by the other side).  Both: a draw.  Neither:
// exactly one side chases perpetually -> that side loses, cause chase; else a draw.
template <typename KeyAt, typename ChkAt, typename RecAt>
__device__ __forceinline__ int wave_repetition_chase_at(KeyAt key_at, ChkAt chk_at, RecAt rec_at, int n, int w, uint64_t key_n, bool chk_n,
                                                        const uint64_t (&rec_n)[4], int side_n, int fold, int lane, int &first, int &cause) {
    bool red, black;
    const int v = wave_repetition_at(key_at, chk_at, n, w, key_n, chk_n, side_n, fold, lane, first, red, black);
    cause = CZ_CAUSE_NONE;
    if (v == CZ_REP_NONE) return v;
    if (v != CZ_REP_DRAW) { cause = CZ_CAUSE_CHECK; return v; }
    if (red) return v;   // both checked
    const int ch = wave_chase_at(rec_at, n, first, rec_n, side_n, lane);
    if (ch == 0 || ch == 3) return CZ_REP_DRAW;
    cause = CZ_CAUSE_CHASE;
    return ch == 1 ? CZ_REP_RED_LOSES : CZ_REP_BLACK_LOSES;
}
__device__ __forceinline__ int wave_repetition_chase(const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check,
                                                     const uint64_t *__restrict__ chase, int imask, int n, int w, uint64_t key_n,
                                                     bool chk_n, const uint64_t (&rec_n)[4], int side_n, int fold, int lane, int &first,
                                                     int &cause) {
    return wave_repetition_chase_at([=](int i) { return keys[i & imask]; }, [=](int i) { return in_check[i & imask] != 0; },
                                    [=](int i, uint64_t &r0, uint64_t &r1, uint64_t &r2, uint64_t &r3) {
                                        const uint64_t *p = chase + (size_t)(i & imask) * 4;
                                        r0 = p[0]; r1 = p[1]; r2 = p[2]; r3 = p[3];
                                    },
                                    n, w, key_n, chk_n, rec_n, side_n, fold, lane, first, cause);
}
