// cz_repmoves.h — TWO-PLY REPETITION VERDICTS ON ROOT MOVES (include/cchess_hip.h: cz_repetition_moves; the specification is
// tests/repmoves_model.py): every king-safe move of a position, and every king-safe reply to it, judged by the live repetition
// rule (cz_repetition.h) against the game's history.  One wave64 per game, nothing but the results leaves the chip:
//   1  the root's king-safe list (czk_position, every lane on the same board: the list is wave-uniform);
//   2  in rounds of 64 candidates, one lane = one candidate: the lane makes its child in ITS 90 bytes of LDS, takes the child's
//      key incrementally from the root's (three Zobrist words and the side key), generates the child's king-safe replies into
//      its list row (the same czk_position, now lane-per-position) and takes every grandchild's key the same way;
//   3  every key is compared with the keys of its side to move inside its window — wave-uniform loads, one compare per lane.
//      A position without an equal key has no verdict; most lanes never see one, and this path holds no board, no flag and no
//      chase record of a grandchild;
//   4  a HIT — a candidate or a (candidate, reply) pair with an equal key — is resolved by the whole wave, one after the
//      other: the position's check flag (czk_position) and chase record (czc_position) on the one board, and the verdict walk
//      of wave_repetition_chase_at over the history with the one or two new positions behind it.
// The history comes through CzvHistory: a caller's record or a slot's ring (imask 63), the current position's key, flag and
// record beside it (a slot's ring entry of the current ply is written later, in choose).
#pragma once
#include "cz_chase.h"
#include "cz_posframe.h"
#include "cz_repetition.h"

// one wave's LDS
struct CzvWave {
    uint32_t cb[CZF_BOARD_WORDS + 4];     // the round's 64 children, 90 bytes apart (czf_unpack's layout and its word behind them)
    uint32_t slots[CZK_SCRATCH * 64];     // [word][lane]: czk_position's / czc_position's scratch
    uint32_t lrow[64 * CZF_LROW];         // the children's reply lists, one row per lane
    uint32_t rootw[24];                   // the root board and two zero bytes behind it
    uint32_t gbw[24];                     // the board of the hit that is being resolved
    uint16_t rlist[CZD_MAXMOVES];         // the root's king-safe list
    uint16_t rp[CZD_MAXMOVES];            // per candidate: reply, own verdict, reply verdict, losing
    uint8_t ov[CZD_MAXMOVES], rv[CZD_MAXMOVES], ls[CZD_MAXMOVES];
};
// the tables every wave of a workgroup reads
struct CzvShared {
    __attribute__((aligned(16))) CzmTables T;
    uint16_t sdt[CZ_NLABELS + 2];         // label -> src | dst << 8
    uint64_t Z[15 * CZ_NSQ + 1];          // the Zobrist keys, the side key last
};
__device__ __forceinline__ void czv_load_shared(CzvShared &S, const CzmTables *__restrict__ gtab, const uint16_t *__restrict__ srcdst,
                                                const uint64_t *__restrict__ zob, int tid, int nthreads) {
    for (int i = tid; i < (int)(sizeof(CzmTables) / 16); i += nthreads) reinterpret_cast<uint4 *>(&S.T)[i] = reinterpret_cast<const uint4 *>(gtab)[i];
    for (int i = tid; i < CZ_NLABELS; i += nthreads) S.sdt[i] = srcdst[i];
    for (int i = tid; i <= 15 * CZ_NSQ; i += nthreads) S.Z[i] = zob[i];
}

// A game's history.  Position i < n0 is at keys / chk [i & imask] and chase [(i & imask) * 4]; n0 is the current position with
// key0, chk0, rec0 and window w0 <= n0; no window grows past wcap (63 for a ring, as wave_root_history's).  valid = false: a
// length outside the record — nothing is read and no position has a verdict.
struct CzvHistory {
    const uint64_t *keys;
    const uint8_t *chk;
    const uint64_t *chase;   // NULL without the chase rule
    int imask, n0, w0, wcap;
    uint64_t key0;
    bool chk0, valid;
    uint64_t rec0[4];
};

// Game g's rows (any may be NULL): moves [128], count [1], verdict [128], reply [128], reply_verdict [128], allowed [66], summary [1]
struct CzvOut {
    uint16_t *moves, *count;
    uint8_t *verdict;
    uint16_t *reply;
    uint8_t *reply_verdict;
    uint32_t *allowed;
    uint8_t *summary;
};

template <bool CHASE>
__device__ __forceinline__ void wave_repetition_moves(CzvWave &W, const CzvShared &S, const uint8_t *__restrict__ board, int side,
                                                      const CzvHistory &H, int fold, int lane, const CzvOut &out) {
    uint8_t *const rootb = reinterpret_cast<uint8_t *>(W.rootw);
    uint8_t *const cb8 = reinterpret_cast<uint8_t *>(W.cb);
    uint8_t *const gb8 = reinterpret_cast<uint8_t *>(W.gbw);
    auto scr = [&W, lane](int i) -> uint32_t & { return W.slots[i * 64 + lane]; };
    auto zk = [&S](int code, int sq) -> uint64_t { return code <= 14 ? S.Z[code * CZ_NSQ + sq] : 0ull; };   // k_hash: a byte above 14 is an empty square
    const uint64_t zside = S.Z[15 * CZ_NSQ];
    const int lossM = side ? CZ_REP_BLACK_LOSES : CZ_REP_RED_LOSES, lossO = side ? CZ_REP_RED_LOSES : CZ_REP_BLACK_LOSES;

    CZF_WAVE_FENCE();   // the previous game's rows have been read
    for (int j = lane; j < 96; j += 64) rootb[j] = j < CZ_NSQ ? board[j] : (uint8_t)0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = r * 64 + lane;
        W.rlist[j] = 0xFFFF; W.rp[j] = 0xFFFF; W.ov[j] = 0; W.rv[j] = 0; W.ls[j] = 0;
    }
    CZF_WAVE_FENCE();
    int n;
    {
        uint32_t w[23], pf;
#pragma unroll
        for (int k = 0; k < 23; ++k) w[k] = W.rootw[k];
        uint16_t *const rl = W.rlist;
        n = czk_position<true, false>(w, side, S.T, scr, [rl](int k, int label) { rl[k & 127] = (uint16_t)label; }, [](int, uint32_t) {}, []() {}, &pf);
        n = __builtin_amdgcn_readfirstlane(n);   // every lane ran the same board
    }
    CZF_WAVE_FENCE();
    if (n < 0) {   // a refused board: count 0xFFFF, every other row zero
        if (out.moves) reinterpret_cast<uint32_t *>(out.moves)[lane] = 0u;
        if (out.count && lane == 0) *out.count = 0xFFFF;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int j = r * 64 + lane;
            if (out.verdict) out.verdict[j] = 0;
            if (out.reply) out.reply[j] = 0;
            if (out.reply_verdict) out.reply_verdict[j] = 0;
        }
        if (out.allowed)
            for (int wd = lane; wd < CZ_MASK_WORDS; wd += 64) out.allowed[wd] = 0u;
        if (out.summary && lane == 0) *out.summary = 0;
        return;
    }

    const int n0 = H.n0, L = n0 + 1, imask = H.imask;
    // the window of a candidate that takes nothing, and of a reply that takes nothing to such a candidate; a capture: 0
    const int W1 = H.valid ? min(min(H.w0 + 1, L), H.wcap) : 0, W2 = H.valid ? min(min(W1 + 1, L + 1), H.wcap) : 0;
    const uint64_t *__restrict__ hk = H.keys;
    const uint8_t *__restrict__ hc = H.chk;
    const uint64_t *__restrict__ hr = H.chase;
    const uint64_t key0 = H.key0;
    const bool chk0 = H.chk0;
    const uint64_t r00 = H.rec0[0], r01 = H.rec0[1], r02 = H.rec0[2], r03 = H.rec0[3];

#pragma unroll 1
    for (int r = 0; r * 64 < n; ++r) {
        const int j = r * 64 + lane;
        const bool act = j < n;
        // ---- the lane's child: its board in LDS, its key from the root's
        const int label = act ? W.rlist[j] : 0;
        const int sd = S.sdt[label], from = sd & 0xFF, to = sd >> 8;
        const int pc = rootb[from], cap = rootb[to];
        {
            uint16_t *c16 = reinterpret_cast<uint16_t *>(cb8) + 45 * lane;
            const uint16_t *r16 = reinterpret_cast<const uint16_t *>(rootb);
#pragma unroll
            for (int h = 0; h < 45; ++h) c16[h] = act ? r16[h] : (uint16_t)0;
            CZF_WAVE_FENCE();
            if (act) { cb8[CZ_NSQ * lane + from] = 0; cb8[CZ_NSQ * lane + to] = (uint8_t)pc; }
        }
        CZF_WAVE_FENCE();
        const uint64_t kc = key0 ^ zk(pc, from) ^ zk(pc, to) ^ zk(cap, to) ^ zside;
        uint16_t *const lrow = reinterpret_cast<uint16_t *>(W.lrow + lane * CZF_LROW);
        int nc;
        bool chkc;
        {
            uint32_t cw[23], pfc;
            czf_unpack(W.cb, lane, act, cw);
            nc = czk_position<true, false>(cw, 1 - side, S.T, scr, [lrow](int k, int lb) { lrow[k & 127] = (uint16_t)lb; }, [](int, uint32_t) {}, []() {}, &pfc);
            nc = act ? max(nc, 0) : 0;   // a refused child has no reply (and no flag: pfc is 0)
            chkc = (pfc & CZK_IN_CHECK) != 0u;
        }
        CZF_WAVE_FENCE();
        const int wc = cap ? 0 : W1;
        // ---- the candidate's key against the positions with its side to move: n0 - 1, n0 - 3, ...
        bool hit = false;
        for (int l = 1; l < W1; l += 2) hit |= hk[(n0 - l) & imask] == kc;
        hit = hit && act && cap == 0;
        // ---- its replies' keys against n0, n0 - 2, ...
        int mx = nc;
#pragma unroll
        for (int o = 32; o; o >>= 1) mx = max(mx, __shfl_xor(mx, o, 64));
        unsigned long long hlo = 0ull, hhi = 0ull;
        if (W2 > 1) {
#pragma unroll 1
            for (int t = 0; t < mx; ++t) {
                const bool a = t < nc && cap == 0;
                const int sd2 = S.sdt[a ? lrow[t] : 0], f2 = sd2 & 0xFF, t2 = sd2 >> 8;
                const int pc2 = cb8[CZ_NSQ * lane + f2], cap2 = cb8[CZ_NSQ * lane + t2];
                const uint64_t kg = kc ^ zk(pc2, f2) ^ zk(pc2, t2) ^ zside;
                bool h = kg == key0;
                for (int l = 3; l < W2; l += 2) h |= hk[(n0 + 1 - l) & imask] == kg;
                h = h && a && cap2 == 0;
                if (t < 64) hlo |= (unsigned long long)h << t;
                else hhi |= (unsigned long long)h << (t - 64);
            }
        }

        // ---- a hit, by the whole wave: candidate c (t < 0) or its reply number t -> CZ_REP_*, cause
        auto judge = [&](int c, int t, int &cause) -> int {
            const uint64_t kcc = __shfl(kc, c, 64);
            const bool chc = __shfl((int)chkc, c, 64) != 0;
            const int wcc = __shfl(wc, c, 64);
            CZF_WAVE_FENCE();
            if (lane < 48) reinterpret_cast<uint16_t *>(gb8)[lane] = lane < 45 ? reinterpret_cast<const uint16_t *>(cb8)[45 * c + lane] : (uint16_t)0;
            CZF_WAVE_FENCE();
            uint64_t recC[4] = {0ull, 0ull, 0ull, 0ull}, recG[4] = {0ull, 0ull, 0ull, 0ull}, kg = 0ull;
            bool chg = false;
            int wg = 0;
#pragma unroll 1
            for (int ph = 0; ph < (t >= 0 ? 2 : 1); ++ph) {   // the child, then the grandchild
                if (ph) {
                    const int sd2 = S.sdt[reinterpret_cast<const uint16_t *>(W.lrow + c * CZF_LROW)[t]], f2 = sd2 & 0xFF, t2 = sd2 >> 8;
                    const int pc2 = gb8[f2], cap2 = gb8[t2];
                    CZF_WAVE_FENCE();
                    if (lane == 0) { gb8[f2] = 0; gb8[t2] = (uint8_t)pc2; }
                    CZF_WAVE_FENCE();
                    kg = kcc ^ zk(pc2, f2) ^ zk(pc2, t2) ^ zk(cap2, t2) ^ zside;
                    wg = cap2 ? 0 : min(min(wcc + 1, L + 1), H.wcap);
                }
                if (!ph && !CHASE) continue;
                uint32_t w[23];
#pragma unroll
                for (int k = 0; k < 23; ++k) w[k] = W.gbw[k];
                if (ph) {
                    uint32_t pfg;
                    czk_position<false, false>(w, side, S.T, scr, [](int, int) {}, [](int, uint32_t) {}, []() {}, &pfg);
                    chg = (pfg & CZK_IN_CHECK) != 0u;
                }
                if constexpr (CHASE) {
                    uint64_t rec[4];
                    czc_position(w, ph ? side : 1 - side, S.T, scr, rec);
#pragma unroll
                    for (int k = 0; k < 4; ++k) { if (ph) recG[k] = rec[k]; else recC[k] = rec[k]; }
                }
            }
            // the history with the child (position L) behind it; the current position's entry comes from H
            auto key_at = [=](int i) -> uint64_t { return i > n0 ? kcc : (i == n0 ? key0 : hk[i & imask]); };
            auto chk_at = [=](int i) -> bool { return i > n0 ? chc : (i == n0 ? chk0 : hc[i & imask] != 0); };
            const uint64_t c0 = recC[0], c1 = recC[1], c2 = recC[2], c3 = recC[3];
            auto rec_at = [=](int i, uint64_t &q0, uint64_t &q1, uint64_t &q2, uint64_t &q3) {
                if (i > n0) { q0 = c0; q1 = c1; q2 = c2; q3 = c3; }
                else if (i == n0) { q0 = r00; q1 = r01; q2 = r02; q3 = r03; }
                else { const uint64_t *p = hr + (size_t)(i & imask) * 4; q0 = p[0]; q1 = p[1]; q2 = p[2]; q3 = p[3]; }
            };
            const int nn = t >= 0 ? L + 1 : L, ww = t >= 0 ? wg : wcc, sn = t >= 0 ? side : 1 - side;
            const uint64_t kn = t >= 0 ? kg : kcc;
            const bool cn = t >= 0 ? chg : chc;
            int first, v;
            if constexpr (CHASE) {
                const uint64_t rn[4] = {t >= 0 ? recG[0] : recC[0], t >= 0 ? recG[1] : recC[1], t >= 0 ? recG[2] : recC[2], t >= 0 ? recG[3] : recC[3]};
                v = wave_repetition_chase_at(key_at, chk_at, rec_at, nn, ww, kn, cn, rn, sn, fold, lane, first, cause);
            } else {
                bool red, black;
                v = wave_repetition_at(key_at, chk_at, nn, ww, kn, cn, sn, fold, lane, first, red, black);
                cause = (v == CZ_REP_RED_LOSES || v == CZ_REP_BLACK_LOSES) ? CZ_CAUSE_CHECK : CZ_CAUSE_NONE;
            }
            return v;
        };

        int ownv = 0, rpl = 0xFFFF, rpv = 0;
        for (unsigned long long m = __ballot(hit); m; m &= m - 1ull) {
            const int c = __ffsll((long long)m) - 1;
            int cause;
            const int v = judge(c, -1, cause);
            if (lane == c) ownv = v | (cause << 4);
        }
        for (;;) {   // the replies in generation order, up to the first that loses
            const unsigned long long pm = __ballot((hlo | hhi) != 0ull);
            if (!pm) break;
            const int c = __ffsll((long long)pm) - 1;
            const unsigned long long lo = __shfl(hlo, c, 64), hi = __shfl(hhi, c, 64);
            const int t = lo ? __ffsll((long long)lo) - 1 : 63 + __ffsll((long long)hi);
            int cause;
            const int v = judge(c, t, cause);
            if (lane == c) {
                if (v == lossM) { rpl = lrow[t & 127]; rpv = v | (cause << 4); hlo = hhi = 0ull; }
                else if (t < 64) hlo &= ~(1ull << t);
                else hhi &= ~(1ull << (t - 64));
            }
        }
        if (act) {
            W.ov[j] = (uint8_t)ownv; W.rp[j] = (uint16_t)rpl; W.rv[j] = (uint8_t)rpv;
            W.ls[j] = ((ownv & 15) == lossM || ((ownv & 15) == CZ_REP_NONE && rpv != 0)) ? 1 : 0;
        }
        CZF_WAVE_FENCE();
    }

    // ---- the rows
    int nlose = 0;
    bool opp = false;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = r * 64 + lane;
        nlose += __popcll(__ballot(W.ls[j] != 0));
        opp |= __ballot(j < n && (W.ov[j] & 15) == lossO) != 0ull;
        if (out.verdict) out.verdict[j] = W.ov[j];
        if (out.reply) out.reply[j] = W.rp[j];
        if (out.reply_verdict) out.reply_verdict[j] = W.rv[j];
    }
    const bool forced = n > 0 && nlose == n, removed = nlose > 0 && !forced;   // a forced loss is still a move
    if (out.moves) reinterpret_cast<uint32_t *>(out.moves)[lane] = reinterpret_cast<const uint32_t *>(W.rlist)[lane];
    if (out.count && lane == 0) *out.count = (uint16_t)n;
    if (out.summary && lane == 0) *out.summary = (uint8_t)((removed ? CZ_REPMOVES_REMOVED : 0) | (forced ? CZ_REPMOVES_FORCED : 0) | (opp ? CZ_REPMOVES_OPP_LOSES : 0));
    if (out.allowed) {   // a lane builds whole words: every label of the list that falls into its word
        for (int wd = lane; wd < CZ_MASK_WORDS; wd += 64) {
            uint32_t x = 0u;
            for (int j = 0; j < n; ++j) {
                const int lb = W.rlist[j];
                if ((lb >> 5) == wd && !(removed && W.ls[j])) x |= 1u << (lb & 31);
            }
            out.allowed[wd] = x;
        }
    }
}
