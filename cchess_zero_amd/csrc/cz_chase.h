// cz_chase.h — the ATTACK-AND-PROTECTION analysis of the perpetual-chase rule (include/cchess_hip.h: cz_threats; the
// specification is tests/chase_model.py).  s is the side to move, the possible victim; X = 1 - s the side that just moved.
// Square t is THREATENED when it holds a piece of s and some pseudo-legal capture a x t of X on this board passes five clauses:
//   1  the attacker is a rook, cannon, knight, advisor or bishop (kings and pawns may chase freely);
//   2  the victim is not the king and not a pawn on its own side of the river;
//   3  the capture is king-safe for X (a pinned piece threatens nothing);
//   4  it is no exchange offer: attacker and victim of one kind, and the victim reaches a on this board;
//   5  the victim is not protected — after a x t, s has a pseudo-legal move onto t (pseudo-legal ON PURPOSE: a pinned
//      protector protects; this is the library's definition) — unless it is worth more than the attacker (R 3, N = C 2,
//      A = B = P 1).
// One lane owns one position, as in cz_kingsafe.h, and the pieces are ITS slots of side X (czk_fill_slots: square + payload
// field in 17 words of per-position scratch), walked in a loop with a wave-uniform switch on the slot's kind.  A slot's capture
// candidates are its field ANDed with the same field layout of the victim squares (clause 2 is part of that set), so a lane
// walks its captures only — a position has two or three; each costs at most three czk_attacked, under CZM_ANY.
// Clauses 4 and 5 ask czk_attacked with fly = false: attackers of an ARBITRARY square, where the king takes one step and does
// not fly.
// Host-compilable like cz_kingsafe.h (tests/chase_host.cpp).
#pragma once
#include "cz_kingsafe.h"

#define CZC_SCRATCH CZK_SLOTS   // words of scratch per position: the slots

CZM_FN CzmSet czc_bit(int q) { return CzmSet{q < 64 ? 1ull << (q & 63) : 0ull, q >= 64 ? 1u << (q & 31) : 0u}; }

// out[0], out[1]: the threatened set (squares 0 .. 63, 64 .. 89); out[2], out[3]: the squares of the side to move.  A board
// the generators refuse (czm_not_a_set of either side, an advisor / bishop move of X without a label) answers four zero words
// and returns false.
template <typename Scr>
CZM_FN bool czc_position(const uint32_t (&w)[23], int side, const CzmTables &T, Scr scr, uint64_t (&out)[4]) {
    const int X = 1 - side;
    CzmSet occ, cand, own;
    CzkPieces vic;
    int kq;
    bool err;
    {
        const CzmSets S = czm_sets(w, X);      // the slots are X's: the side NOT to move
        err = czm_not_a_set(S);
        kq = czm_lowest(S.K);
        czk_fill_slots(S, X, T, scr);
        occ = S.occ;
    }
    {
        const CzmSets V = czm_sets(w, side);
        err |= czm_not_a_set(V);
        vic = czk_pieces(V);
        own = V.own;
        // clause 2: not the king, not a pawn on its own side of the river (red: y <= 4, squares 0 .. 44; black: y >= 5)
        const CzmSet home = side ? CzmSet{~((1ull << 45) - 1ull), 0x03FFFFFFu} : CzmSet{(1ull << 45) - 1ull, 0u};
        cand = CzmSet{V.own.lo & ~V.K.lo & ~(V.P.lo & home.lo), V.own.hi & ~V.K.hi & ~(V.P.hi & home.hi)};
    }
#pragma unroll 1
    for (int s = 12; s < 16; ++s) {   // an advisor / bishop move without a label: refused, as czk_position does
        const uint32_t v = scr(s);
#pragma unroll
        for (int d = 0; d < 4; ++d) err |= ((czk_slot_field(v) >> d) & 1u) != 0u && T.ab[s >= 14 ? 1 : 0][czk_slot_sq(v) * 4 + d] == 0xFFu;
    }
    CzmSet threat = {0ull, 0u};
#pragma unroll 1
    for (int s = 0; s < 16; ++s) {
        if (s >= 6 && s < 12) continue;   // clause 1: the king (and the flying general, slot 16) and the pawns
        const uint32_t v = scr(s);
        const int a = czk_slot_sq(v), ay = a / 9, ax = a - ay * 9;
        // the slot's victims in the layout of its field; aval: the attacker's value
        uint32_t vf;
        int aval;
        if (s < 4) {
            vf = czm_ortho_field(czm_rank(cand, ay), czm_file(cand, ax), ax, ay);
            aval = s < 2 ? 3 : 2;
        } else if (s < 6) {               // czm_knight_good's window: jump j lands on bit 19 + 9 dy + dx
            const uint64_t nw = czm_window(cand, a - 19);
            vf = czm_wbit(nw, 8) | (czm_wbit(nw, 0) << 1) | (czm_wbit(nw, 26) << 2) | (czm_wbit(nw, 2) << 3) |
                 (czm_wbit(nw, 12) << 4) | (czm_wbit(nw, 36) << 5) | (czm_wbit(nw, 30) << 6) | (czm_wbit(nw, 38) << 7);
            aval = 2;
        } else {                          // czm_diag_good's window: direction d lands on bit 20 + st (9 sy + sx)
            const uint64_t dw = czm_window(cand, a - 20);
            vf = s < 14 ? czm_wbit(dw, 10) | (czm_wbit(dw, 12) << 1) | (czm_wbit(dw, 30) << 2) | (czm_wbit(dw, 28) << 3)
                        : czm_wbit(dw, 0) | (czm_wbit(dw, 4) << 1) | (czm_wbit(dw, 40) << 2) | (czm_wbit(dw, 36) << 3);
            aval = 1;
        }
        uint32_t left = err ? 0u : czk_slot_field(v) & vf;   // a field bit is a pseudo-legal move: on the board, no wrap
        if (!CZM_ANY(left != 0u)) continue;
        const CzmSet occ2 = czm_without(occ, a);             // after a x t: a is empty, t stays occupied
        while (CZM_ANY(left != 0u)) {   // every lane walks ITS captures, lowest bit first (czk_filter's walk)
            const bool b = left != 0u;
            const int i = b ? czm_ctz32(left) : 0;
            left &= left - 1u;
            const int t = b ? czk_dest(s, a, i) : 0;
            bool live = b && !czm_tst(threat, t);            // a square another attacker threatens already needs no second look
            // the victim's kind by bit tests (a set picked by the slot's kind would be an array indexed at run time)
            const bool vR = czm_tst(vic.R, t), vC = czm_tst(vic.C, t), vN = czm_tst(vic.N, t), vA = czm_tst(vic.A, t), vB = czm_tst(vic.B, t);
            const bool kin = s < 2 ? vR : (s < 4 ? vC : (s < 6 ? vN : (s < 14 ? vA : vB)));
            const bool guard = (vR ? 3 : ((vN | vC) ? 2 : 1)) <= aval;   // a protector saves only a victim that is worth no more
            const CzmSet tb = czc_bit(t);
            // the three questions, one after the other through ONE copy of czk_attacked (a wave-uniform phase):
            //   clause 3  is X's king attacked after a x t?            occ - a, s's pieces without t, the king's square, flying general
            //   clause 4  does the victim itself reach a as it stands?  occ,     s's piece on t alone,  a
            //   clause 5  does s reach t after a x t?                   occ - a, s's pieces without t, t
#pragma unroll 1
            for (int ph = 0; ph < 3; ++ph) {
                const bool ask = live && (ph == 0 ? kq >= 0 : (ph == 1 ? kin : guard));
                if (!CZM_ANY(ask)) continue;
                if (ask) {
                    const CzmSet m = ph == 1 ? tb : CzmSet{~tb.lo, ~tb.hi};
                    const CzkPieces p = {czm_and(vic.R, m), czm_and(vic.C, m), czm_and(vic.N, m), czm_and(vic.P, m), czm_and(vic.K, m),
                                         czm_and(vic.A, m), czm_and(vic.B, m)};
                    const int k = ph == 0 ? kq : (ph == 1 ? a : t);
                    live = !czk_attacked(ph == 1 ? occ : occ2, p, side, k, T.knon[k], ph == 0);
                }
            }
            if (live) { threat.lo |= tb.lo; threat.hi |= tb.hi; }
        }
    }
    out[0] = err ? 0ull : threat.lo;
    out[1] = err ? 0ull : (uint64_t)threat.hi;
    out[2] = err ? 0ull : own.lo;
    out[3] = err ? 0ull : (uint64_t)own.hi;
    return !err;
}
