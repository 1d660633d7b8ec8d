// cz_kingsafe.h — KING-SAFE move generation: the pseudo-legal moves of cz_maskgen.h (GameBoard.get_legal_moves, main.py:743-1109)
// without those that leave the mover's king attacked, plus the position's check flags.  The reference has no such function: its
// games end when a king is taken.  The definition rests on its generator alone (tests/kingsafe_model.py):
//   attacked(board, s)  = s has a king and the other side has a pseudo-legal move onto its square (the flying general of
//                         main.py:1097-1107 is such a move);
//   m is king-safe      = not attacked(board after m, mover) — one rule, also for moves that take the enemy king and for boards
//                         without a king of the mover (every move is safe there).
// One lane owns one position, as in czm_position / czm_list, and the pieces are the same 16 slots with the same payload fields
// (built from the same czm_* functions, which this header only calls).  What is new:
//   * czk_attacked: is square k attacked?  Looked at FROM k: the first and second occupied square of its rank and file in both
//     directions (rook / king, cannon), the eight knight squares with their legs (k's diagonal neighbours), the three pawn squares,
//     and — for a king that an arbitrary board puts into the other side's half — advisor, bishop and king steps.  No enemy move
//     is generated.
//   * czk_filter: the 17 fields (16 slots + the flying general) slot by slot, every lane walking the set bits of its own field;
//     a move of another piece than the king whose source and destination lie off k's rank, file and 5 x 5 neighbourhood cannot
//     change whether k is attacked, so it keeps the position's own answer without a test, and a step of the walk that no lane
//     of the wave has to test is skipped (CZM_ANY).
//   * the slots live in 34 words of per-position scratch (scr(i), like czm_list's), so that the walk over slots is a LOOP
//     with a wave-uniform switch on the slot's kind: one copy of czk_attacked in the code, no register arrays indexed at run time.
// Host-compilable like cz_maskgen.h (tests/kingsafe_host.cpp).
#pragma once
#include "cz_maskgen.h"

#define CZK_IN_CHECK 1u        // CZ_POS_IN_CHECK: attacked(board, side)
#define CZK_CAN_TAKE_KING 2u   // CZ_POS_CAN_TAKE_KING: attacked(board, 1 - side)
#define CZK_NO_SAFE_MOVE 4u    // CZ_POS_NO_SAFE_MOVE: the king-safe list is empty
#define CZK_SLOTS 17           // czm_list's 16 piece slots + the flying general (source: the king's square)
#define CZK_SCRATCH 34         // words of scratch per position: the slots, then 17 for the list offsets

struct CzkPieces { CzmSet R, C, N, P, K, A, B; };   // one side's pieces by kind
CZM_FN CzkPieces czk_pieces(const CzmSets &S) { return CzkPieces{S.R, S.C, S.N, S.P, S.K, S.A, S.B}; }
CZM_FN CzkPieces czk_without(const CzkPieces &p, int q) {
    return CzkPieces{czm_without(p.R, q), czm_without(p.C, q), czm_without(p.N, q), czm_without(p.P, q), czm_without(p.K, q), czm_without(p.A, q), czm_without(p.B, q)};
}

// Is square k attacked by the pieces `a` of side `as` (0 = red) on the occupancy `occ`?  knon = CzmTables::knon[k].
// fly (the default, and what every king-safe caller asks): k holds a king, so the attacker's king anywhere on k's file with
// nothing between takes it (the flying general).  fly = false is the question for ANY occupied square (cz_chase.h: is a piece
// protected, does a piece reach its attacker): the attacker's king reaches k by one step inside its palace and in no other way.
// (A run-time flag, wave-uniform where it is not a constant: cz_chase.h asks both questions from ONE copy of this function.)
CZM_FN bool czk_attacked(const CzmSet &occ, const CzkPieces &a, int as, int k, uint32_t knon, bool fly = true) {
    const int y = k / 9, x = k - y * 9;
    // rank and file: czm_line_dests with every square an enemy is the run up to and including the first occupied square (rook),
    // resp. the second occupied square behind one screen (cannon); the king's own bit is part of occ, as a slider's is
    const uint32_t ro = czm_rank(occ, y), fo = czm_file(occ, x);
    const uint32_t r1 = czm_line_dests<false>(ro, ~0u, x, 9) & ro, f1 = czm_line_dests<false>(fo, ~0u, y, 10) & fo;
    const uint32_t r2 = czm_line_dests<true>(ro, ~0u, x, 9) & ro, f2 = czm_line_dests<true>(fo, ~0u, y, 10) & fo;
    const uint32_t kr = czm_rank(a.K, y);
    const uint32_t kf = czm_file(a.K, x);
    uint32_t hit = (r1 & czm_rank(a.R, y)) | (f1 & (czm_file(a.R, x) | (fly ? kf : 0u))) |   // a king on the file with nothing between: the flying general
                   (r2 & czm_rank(a.C, y)) | (f2 & czm_file(a.C, x));
    // knight on k + (dx, dy): bit 19 + 9 dy + dx of the window at k - 19 (czm_knight_good's positions); its leg is k's diagonal
    // neighbour on that side: bits 9, 11, 27, 29
    {
        const uint64_t nw = czm_window(a.N, k - 19), em = ~czm_window(occ, k - 19);
        const uint32_t at = czm_wbit(nw, 8) | (czm_wbit(nw, 0) << 1) | (czm_wbit(nw, 26) << 2) | (czm_wbit(nw, 2) << 3) |
                            (czm_wbit(nw, 12) << 4) | (czm_wbit(nw, 36) << 5) | (czm_wbit(nw, 30) << 6) | (czm_wbit(nw, 38) << 7);
        const uint32_t lg = (czm_wbit(em, 9) * 0x03u) | (czm_wbit(em, 11) * 0x18u) | (czm_wbit(em, 27) * 0x24u) | (czm_wbit(em, 29) * 0xC0u);
        hit |= at & lg & knon;
    }
    // pawn (main.py:1063-1095): red steps to y + 1, black to y - 1; sideways from beyond the river (the pawn's rank is k's)
    {
        const uint64_t pw = czm_window(a.P, k - 9);   // bit 0: k - 9, 8: k - 1, 10: k + 1, 18: k + 9
        const bool river = as ? y < 5 : y > 4;
        hit |= as ? czm_wbit(pw, 18) : czm_wbit(pw, 0);
        hit |= (uint32_t)(river & (x >= 1)) & czm_wbit(pw, 8);
        hit |= (uint32_t)(river & (x <= 7)) & czm_wbit(pw, 10);
    }
    // Advisors, bishops and the king's own steps reach k only inside the attacker's half of the board, where no game puts the
    // other king; an arbitrary board may (the generator restricts the TARGET square alone: czm_diag_good, czm_king_field)
    const bool half = as ? y >= 5 : y <= 4;
    if (CZM_ANY(half)) {
        const bool palace = (as ? y >= 7 : y <= 2) & (x >= 3) & (x <= 5);
        const uint64_t aw = czm_window(a.A, k - 10);   // bit 0: k - 10, 2: k - 8, 18: k + 8, 20: k + 10; x is 3 .. 5: no wrap
        const uint32_t adv = czm_wbit(aw, 0) | czm_wbit(aw, 2) | czm_wbit(aw, 18) | czm_wbit(aw, 20);
        uint32_t kst = ((kr << 1) | (kr >> 1)) >> x & 1u;   // the attacker's king on k - 1 or k + 1 (k +- 9 is on the file: above)
        if (!fly) kst |= ((kf << 1) | (kf >> 1)) >> y & 1u;  // without the flying general k +- 9 is a step like the other two
        hit |= (uint32_t)palace & (adv | kst);
        const uint64_t bw = czm_window(a.B, k - 20), ew = ~czm_window(occ, k - 20);   // bishop: bit 20 + 2 (9 sy + sx), eye: bit 20 + 9 sy + sx
        const uint32_t bl = (czm_wbit(bw, 0) & czm_wbit(ew, 10)) | (czm_wbit(bw, 36) & czm_wbit(ew, 28));   // dx = -2
        const uint32_t br = (czm_wbit(bw, 4) & czm_wbit(ew, 12)) | (czm_wbit(bw, 40) & czm_wbit(ew, 30));   // dx = +2
        hit |= (uint32_t)half & (((uint32_t)(x >= 2) & bl) | ((uint32_t)(x <= 6) & br));
    }
    return hit != 0u;
}

// ---- the slots: czm_list's 16 (square, payload field) pairs + the flying general, one scratch word each: field << 8 | square
CZM_FN int czk_slot_sq(uint32_t v) { return (int)(v & 0xFFu); }
CZM_FN uint32_t czk_slot_field(uint32_t v) { return v >> 8; }
// kinds of the slots: 0, 1 rooks; 2, 3 cannons; 4, 5 knights; 6 king; 7 .. 11 pawns; 12, 13 advisors; 14, 15 bishops; 16 flying general
template <typename Scr>
CZM_FN void czk_fill_slots(const CzmSets &S, int side, const CzmTables &T, Scr scr) {
    auto slot = [&](int s, int sq, bool ok, uint32_t f) { scr(s) = ok ? (f << 8) | (uint32_t)sq : 0u; };
    auto sq_or_0 = [](int sq, bool ok) { return ok ? sq : 0; };
    const int lo[6] = {czm_lowest(S.R), czm_lowest(S.C), czm_lowest(S.N), czm_lowest(S.A), czm_lowest(S.B), czm_lowest(S.K)};
    const int hi[5] = {czm_highest(S.R), czm_highest(S.C), czm_highest(S.N), czm_highest(S.A), czm_highest(S.B)};
#pragma unroll
    for (int it = 0; it < 2; ++it) {   // the lowest and the highest square of each kind (czm_not_a_set refuses a third piece)
        bool ok[5];
        int q[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { ok[k] = it ? hi[k] > lo[k] : lo[k] >= 0; q[k] = sq_or_0(it ? hi[k] : lo[k], ok[k]); }
        slot(0 + it, q[0], ok[0], czm_slider_field<false>(S, q[0]));
        slot(2 + it, q[1], ok[1], czm_slider_field<true>(S, q[1]));
        slot(4 + it, q[2], ok[2], czm_knight_good(S, q[2], T.knon[q[2]]));
        slot(12 + it, q[3], ok[3], czm_diag_good<0>(S, side, q[3]));
        slot(14 + it, q[4], ok[4], czm_diag_good<1>(S, side, q[4]));
    }
    {
        const bool ok = lo[5] >= 0;
        uint32_t fg;
        const uint32_t f = czm_king_field(S, side, sq_or_0(lo[5], ok), czm_lowest(S.EK), &fg);
        slot(6, lo[5], ok, f);
        slot(16, lo[5], ok, fg);
    }
    const CzmPawnSets PS = czm_pawn_sets(S, side);
    CzmSet P = S.P;
#pragma unroll 1
    for (int it = 0; it < 5; ++it) {
        const int sq = czm_lowest(P);
        P = czm_without(P, sq);
        slot(7 + it, sq, sq >= 0, czm_pawn_field2(PS, side, sq_or_0(sq, sq >= 0)));
    }
}
// the destination square of bit i of the field of slot s, a piece on q (wave-uniform switch on the slot)
CZM_FN int czk_dest(int s, int q, int i) {
    const int y = q / 9, x = q - y * 9;
    if (s >= 4 && s < 6)     // knight jump i of the vocabulary order: (dx, dy) = (-2,-1) (-1,-2) (-2,1) (1,-2) (2,-1) (-1,2) (2,1) (1,2)
        return q - 19 + (int)((0x261E240C021A0008ull >> (8 * i)) & 0xFFu);   // 19 + 9 dy + dx, a byte per jump
    if (s >= 12 && s < 16) { // diagonal i: (dy, dx) = (-s,-s) (-s,+s) (+s,+s) (+s,-s)
        const int d = (int)((0x12140200u >> (8 * i)) & 0xFFu) - 10;        // 9 dy + dx + 10 for one step: -10, -8, +10, +8
        return q + (s >= 14 ? 2 * d : d);
    }
    // the 17-bit field of czm_ortho_field: bits 0 .. 7 the other files of the rank, 8 .. 16 the other ranks of the file
    const int j = i - 8;
    return i < 8 ? 9 * y + (i < x ? i : i + 1) : 9 * (j < y ? j : j + 1) + x;
}

// Is sq on the rank or the file of the king on (ky, kx) or within two files and ranks of it?  A superset of the squares
// czk_attacked reads for that king.
CZM_FN bool czk_near(int sq, int ky, int kx) {
    const int y = sq / 9, x = sq - y * 9, dy = y - ky, dx = x - kx;
    return (dy == 0) | (dx == 0) | ((dy >= -2) & (dy <= 2) & (dx >= -2) & (dx <= 2));
}
// the set with its piece on q moved to dst
CZM_FN CzmSet czk_moved(const CzmSet &s, int q, int dst) {
    const CzmSet w = czm_without(s, q);
    return CzmSet{w.lo | (dst < 64 ? 1ull << (dst & 63) : 0ull), w.hi | (dst >= 64 ? 1u << (dst & 31) : 0u)};
}

// The filter: clears the bits of the moves that are not king-safe in every slot; returns the number of moves left.
// kq: the mover's king (-1: none, nothing is cleared); in_check = attacked(board, side).
template <typename Scr>
CZM_FN int czk_filter(const CzmSets &S, const CzkPieces &enemy, int side, const CzmTables &T, int kq, bool in_check, Scr scr) {
    const int ky = (kq >= 0 ? kq : 0) / 9, kx = (kq >= 0 ? kq : 0) - 9 * ky;
    auto sensitive = [&](int sq) { return czk_near(sq, ky, kx); };
    int total = 0;
#pragma unroll 1
    for (int s = 0; s < CZK_SLOTS; ++s) {
        const uint32_t v = scr(s);
        const int q = czk_slot_sq(v);
        uint32_t f = czk_slot_field(v);
        const bool king = (s == 6) | (s == 16), from = king | sensitive(q);
        // every lane walks the set bits of ITS field (lowest first): the slot takes as many steps as its richest field in the wave
        // has moves (a pawn 3, a king 4, a rook ~12) — a fixed walk over the 17 bit positions took 219 steps per position, this
        // one ~90 (1.82 -> 1.42 ms per 1 M positions); czk_dest is arithmetic on the lane's own bit index.  czm_list's
        // round-6 lesson was about ONE such loop over a whole position's moves (~140 steps); here the bound is a single field
        uint32_t left = kq >= 0 ? f : 0u;
        if (CZM_ANY(left != 0u)) {
            while (CZM_ANY(left != 0u)) {
                const bool b = left != 0u;
                const int i = b ? czm_ctz32(left) : 0;
                left &= left - 1u;
                const int dst = b ? czk_dest(s, q, i) : 0;
                const bool test = b && (from | sensitive(dst));
                bool bad = b & !test & in_check;   // nothing k's attackers see has moved: the position's own answer
                if (CZM_ANY(test)) {
                    if (test) {
                        const int k = king ? dst : kq;
                        bad = czk_attacked(czk_moved(S.occ, q, dst), czk_without(enemy, dst), 1 - side, k, T.knon[k]);
                    }
                }
                f &= ~((uint32_t)bad << i);
            }
            scr(s) = (f << 8) | (uint32_t)q;
        }
        total += __builtin_popcount(f);
    }
    return total;
}

// The checks: a second pass over the FILTERED slots that clears every move after which the other king is not attacked, so
// that the slots hold the king-safe moves that give check; returns their number.  eq: the other king (-1: none, no move gives
// check); can_take = attacked(board, 1 - side).  The test is the filter's, seen from the other king: czk_attacked for eq on
// the occupancy and the MOVER's pieces after the move.  A move that takes that king gives no check (a side without a king is
// not attacked) — the flying general of slot 16 is always one —, and a move whose source and destination lie off eq's rank,
// file and 5 x 5 neighbourhood changes nothing czk_attacked reads: it keeps the position's own answer, can_take.
template <typename Scr>
CZM_FN int czk_checks(const CzmSets &S, const CzkPieces &mine, int side, const CzmTables &T, int eq, bool can_take, Scr scr) {
    const int e = eq >= 0 ? eq : 0, ey = e / 9, ex = e - 9 * ey;
    const uint32_t knon = T.knon[e];
    int total = 0;
#pragma unroll 1
    for (int s = 0; s < CZK_SLOTS; ++s) {
        const uint32_t v = scr(s);
        const int q = czk_slot_sq(v);
        uint32_t f = czk_slot_field(v);
        const bool from = czk_near(q, ey, ex);
        uint32_t left = f;
        if (CZM_ANY(left != 0u)) {
            while (CZM_ANY(left != 0u)) {   // every lane walks the set bits of its field, as in czk_filter
                const bool b = left != 0u;
                const int i = b ? czm_ctz32(left) : 0;
                left &= left - 1u;
                const int dst = b ? czk_dest(s, q, i) : 0;
                const bool live = b && eq >= 0 && dst != eq;
                const bool test = live && (from | czk_near(dst, ey, ex));
                bool chk = live & !test & can_take;
                if (CZM_ANY(test)) {
                    if (test) {
                        CzkPieces m = mine;   // the slot's kind is wave-uniform: one of the seven sets moves
                        if (s < 2) m.R = czk_moved(mine.R, q, dst);
                        else if (s < 4) m.C = czk_moved(mine.C, q, dst);
                        else if (s < 6) m.N = czk_moved(mine.N, q, dst);
                        else if (s == 6 || s == 16) m.K = czk_moved(mine.K, q, dst);
                        else if (s < 12) m.P = czk_moved(mine.P, q, dst);
                        else if (s < 14) m.A = czk_moved(mine.A, q, dst);
                        else m.B = czk_moved(mine.B, q, dst);
                        chk = czk_attacked(czk_moved(S.occ, q, dst), m, side, e, knon);
                    }
                }
                f &= ~((uint32_t)(b & !chk) << i);
            }
            scr(s) = (f << 8) | (uint32_t)q;
        }
        total += __builtin_popcount(f);
    }
    return total;
}

// The SET of the (filtered) slots: czm_position's 15 (bit, field) pairs, in its order
template <typename Scr, typename Emit>
CZM_FN void czk_emit_set(const CzmTables &T, Scr scr, Emit emit) {
    const uint32_t fg = czk_slot_field(scr(16));
    uint64_t lits = 0ull;
#pragma unroll 1
    for (int s = 0; s < 16; ++s) {
        const uint32_t v = scr(s);
        const int q = czk_slot_sq(v);
        const uint32_t f = czk_slot_field(v);
        if (s >= 12) {           // advisor / bishop literals
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const uint32_t l = T.ab[s >= 14 ? 1 : 0][q * 4 + d];
                lits |= (((f >> d) & 1u) != 0u && l != 0xFFu) ? 1ull << (l & 63u) : 0ull;
            }
        } else if (s >= 4 && s < 6) {   // knight: the vocabulary lists the on-board jumps only
            const uint32_t on = T.knon[q];
            uint32_t c = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) c |= ((f >> j) & 1u) << __builtin_popcount(on & czm_low(j));
            emit((int)T.base[q] + 17, c);
        } else {
            emit((int)T.base[q], s == 6 ? f | fg : f);
        }
    }
    emit(CZM_NLIT_BASE, (uint32_t)lits & 0xFFFFu);
    emit(CZM_NLIT_BASE + 16, (uint32_t)(lits >> 16) & 0xFFFFu);
    emit(CZM_NLIT_BASE + 32, (uint32_t)(lits >> 32) & 0xFFFFu);
}

// The ORDERED LIST of the (filtered) slots, in the reference's order (see czm_list): pieces by ascending square, each its
// candidates in get_legal_moves' order, the flying general last.  put(n, label): `label` is move number n.  A piece's place is
// the sum of the counts of the pieces on lower squares: count written at the piece's rank among the own pieces (scratch words
// 17 .. 33), running sums, read back by rank.
template <typename Scr, typename Put>
CZM_FN void czk_emit_list(const CzmSets &S, const CzmTables &T, int total, Scr scr, Put put) {
    const uint32_t o0 = (uint32_t)S.own.lo, o1 = (uint32_t)(S.own.lo >> 32), o2 = S.own.hi;
    const int p1 = __builtin_popcount(o0), p2 = p1 + __builtin_popcount(o1);
    auto rank = [&](uint32_t v) { return 17 + (czm_rank_below(o0, o1, o2, p1, p2, czk_slot_sq(v)) & 15); };
#pragma unroll 1
    for (int r = 17; r < 34; ++r) scr(r) = 0u;
#pragma unroll 1
    for (int s = 0; s < 16; ++s) {
        const uint32_t v = scr(s), c = (uint32_t)__builtin_popcount(czk_slot_field(v));
        if (c) scr(rank(v)) = c;   // an empty or missing slot would write rank 0: another piece's word
    }
    uint32_t run = 0u;
#pragma unroll 1
    for (int r = 17; r < 33; ++r) { const uint32_t c = scr(r); scr(r) = run; run += c; }
#pragma unroll 1
    for (int s = 0; s < 16; ++s) {
        const uint32_t v = scr(s);
        const int q = czk_slot_sq(v), y = q / 9, x = q - y * 9, base = T.base[q];
        const uint32_t f = czk_slot_field(v);
        int n = (int)scr(rank(v));
        auto cand = [&](uint32_t b, int label) { if (b & 1u) put(n, label); n += (int)(b & 1u); };
        if (!CZM_ANY(f != 0u)) continue;
        if (s < 4 || s == 6) {          // rook / cannon: -x, +x, -y, +y, each from the piece outwards; the king's four steps are the same walk
#pragma unroll 1
            for (int p = 0; p < 8; ++p) { const int i = p < x ? x - 1 - p : p; cand(f >> i, base + i); }
#pragma unroll 1
            for (int p = 0; p < 9; ++p) { const int i = 8 + (p < y ? y - 1 - p : p); cand(f >> i, base + i); }
        } else if (s < 6) {             // knight: (2i, j) then (i, 2j) for i, j in (-1, +1)^2 = vocabulary jumps 1, 0, 3, 4, 5, 2, 7, 6
            const uint32_t on = T.knon[q];
#pragma unroll 1
            for (int o = 0; o < 8; ++o) { const int j = (int)((0x67254301u >> (4 * o)) & 15u); cand(f >> j, base + 17 + __builtin_popcount(on & czm_low(j))); }
        } else if (s < 12) {            // pawn: forward (the one bit of the file field), x + 1, x - 1
            const uint32_t fl = f >> 8;
            cand(fl != 0u ? 1u : 0u, base + 8 + (fl ? czm_ctz32(fl) : 0));
            cand((f & 0xFFu) >> x, base + x);
            cand(((f & 0xFFu) << 1) >> x, base + x - 1);
        } else {                        // advisor / bishop: (-,-) (-,+) (+,+) (+,-)
#pragma unroll 1
            for (int d = 0; d < 4; ++d) {
                const uint32_t l = T.ab[s >= 14 ? 1 : 0][q * 4 + d];
                cand(f >> d, CZM_NLIT_BASE + (int)(l & 63u));
            }
        }
    }
    const uint32_t v = scr(16), fg = czk_slot_field(v);
    if (fg) put(total - 1, (int)T.base[czk_slot_sq(v)] + czm_ctz32(fg));
}

// ---- the position.  scr(i), 0 <= i < CZK_SCRATCH: per-position scratch words; put(n, label) and emit(bit, field) as above,
// called only with LIST / SET; mid() is called once, after the last emit and before the first put (a caller may build the set's
// rows and the list's rows in the same memory, as k_movegen_kingsafe does).  *pos_flags: the CZK_* bits.  Returns the number of king-safe moves, or -1 for a board the
// stand-alone generators refuse (czm_not_a_set, an advisor / bishop move without a label): its flags are 0.
// CHECKS: the list, the set and the number returned are those of the king-safe moves that give check (czk_checks); the flags
// stay the position's own — CZK_NO_SAFE_MOVE speaks of all king-safe moves.
template <bool LIST, bool SET, bool CHECKS = false, typename Scr, typename Put, typename Emit, typename Mid>
CZM_FN int czk_position(const uint32_t (&w)[23], int side, const CzmTables &T, Scr scr, Put put, Emit emit, Mid mid, uint32_t *pos_flags) {
    const CzmSets S = czm_sets(w, side);
    bool err = czm_not_a_set(S);
    const CzkPieces mine = czk_pieces(S), enemy = czk_pieces(czm_sets(w, 1 - side));
    const int kq = czm_lowest(S.K), eq = czm_lowest(S.EK);
    const bool in_check = kq >= 0 && czk_attacked(S.occ, enemy, 1 - side, kq >= 0 ? kq : 0, T.knon[kq >= 0 ? kq : 0]);
    const bool can_take = eq >= 0 && czk_attacked(S.occ, mine, side, eq >= 0 ? eq : 0, T.knon[eq >= 0 ? eq : 0]);
    czk_fill_slots(S, side, T, scr);
    {   // an advisor / bishop move without a label is an error before the filter can clear it (czm_position, czm_list)
#pragma unroll 1
        for (int s = 12; s < 16; ++s) {
            const uint32_t v = scr(s);
#pragma unroll
            for (int d = 0; d < 4; ++d) err |= ((czk_slot_field(v) >> d) & 1u) != 0u && T.ab[s >= 14 ? 1 : 0][czk_slot_sq(v) * 4 + d] == 0xFFu;
        }
    }
    const int total = czk_filter(S, enemy, side, T, kq, in_check, scr);
    const int listed = CHECKS ? czk_checks(S, mine, side, T, eq, can_take, scr) : total;
    if (SET) czk_emit_set(T, scr, emit);
    mid();
    if (LIST) czk_emit_list(S, T, listed, scr, put);
    *pos_flags = err ? 0u : ((in_check ? CZK_IN_CHECK : 0u) | (can_take ? CZK_CAN_TAKE_KING : 0u) | (total == 0 ? CZK_NO_SAFE_MOVE : 0u));
    return err ? -1 : listed;
}
