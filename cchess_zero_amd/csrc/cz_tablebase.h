// cz_tablebase.h — ENDGAME TABLEBASES: the index <-> position mapping of a material class and one index's step of the
// retrograde build.  The reference has no such thing (its games end when a king is taken); the contract is the one of
// include/cchess_hip.h (TABLEBASES) and nothing of the rules is restated here: the moves are czk_position<LIST>'s king-safe
// list (cz_kingsafe.h), a move is srcdst's two squares.
//   signature  "KR-KAA": red letters, '-', black letters, each side in the order KRNCPAB; every letter is a SLOT
//   domain     the squares a slot may stand on, ascending: K 9, A 5, B 7, P 55, R N C 90 (black: y -> 9 - y) — arithmetic both
//              ways (cztb_square, cztb_digit), no table
//   index      2 * mixed_radix(d0, d1, ...) + side, slot 0 the most significant digit, d_i the place of slot i's square
//   value      int16 from the mover's view: 0 draw, v > 0 the mover mates in v - 1 plies, v < 0 it is mated in -v - 1
// One lane owns one index, as one lane owns one position in cz_kingsafe.h: the slots' squares and digits live in
// CZTB_MAX_SLOTS registers each and every loop over them is unrolled with `k < n` as a predicate — a register array is never
// indexed at run time (czg_code, czg_apply); the descriptor is wave-uniform (kernel arguments on the GPU).
// THE CHILD OF A MOVE IS AN INDEX, NOT A BOARD: the slot on `from` takes the digit of `to`, the side flips, and a move that
// takes the piece of slot j leaves digit j out — Horner over the remaining slots is the index in the table of the signature
// without that letter, which keeps the slot order.  Two bytes are read per child.
// A SET OF TABLES (cz_tablebase_set.hip) is found by MATERIAL KEY: cztb_material_key of a board from the planes cztb_rank reads,
// cztb_desc_key of a signature, and the sorted directory of keys (cztb_set_sort, cztb_set_find).
// Host-compilable like cz_games.h (tests/tablebase_host.cpp, tests/tablebase_set_host.cpp): k_tb_pass (cz_tablebase.hip),
// k_tb_probe_set and the host test programs compile this very text.
#pragma once
#include "cz_games.h"

#define CZTB_MAX_SLOTS 10      // 2 kings + the eight smallest domains (AABB on both sides) is the longest signature below 2^31 entries
#define CZTB_ILLEGAL (-32768)  // CZ_TB_ILLEGAL
#define CZTB_UNKNOWN 32767     // CZ_TB_UNKNOWN
#define CZTB_MISS 32766        // CZ_TB_MISS
// domain ids: 0 every square; 1 .. 4 red K A B P; 5 .. 8 black K A B P
#define CZTB_DOM_ALL 0
#define CZTB_DOM_K 1
#define CZTB_DOM_A 2
#define CZTB_DOM_B 3
#define CZTB_DOM_P 4

struct CztbDesc {
    int32_t n;                        // slots
    uint32_t entries;                 // 2 * the product of the radices, <= 2^31 - 1
    uint8_t code[CZTB_MAX_SLOTS];     // the slot's piece code (1 + index in "KARBNPCkarbnpc")
    uint8_t dom[CZTB_MAX_SLOTS];      // its domain id
    uint8_t radix[CZTB_MAX_SLOTS];    // the size of its domain
    uint8_t ord[CZTB_MAX_SLOTS];      // how many earlier slots have the same code: among equal pieces the k-th in ascending square order is the k-th slot
    uint8_t mult[CZTB_MAX_SLOTS];     // how many slots have this slot's code
};

// ---- signatures (host) --------------------------------------------------------------------------------------------------------
// -> 0 and *d, or a negative number: -1 not "<red>-<black>" of the letters KRNCPAB, -2 a side does not start with its one K,
// -3 letters out of order or too many of one (2 of R N C A B, 5 P), -4 more than CZTB_MAX_SLOTS slots or 2^31 - 1 entries
inline int cztb_parse(const char *sig, CztbDesc *d) {
    static const char letters[] = "KRNCPAB";
    static const int code[7] = {1, 3, 5, 7, 6, 2, 4}, dom[7] = {CZTB_DOM_K, 0, 0, 0, CZTB_DOM_P, CZTB_DOM_A, CZTB_DOM_B},
                     radix[7] = {9, 90, 90, 90, 55, 5, 7}, most[7] = {1, 2, 2, 2, 5, 2, 2};
    CztbDesc o;
    o.n = 0;
    for (int k = 0; k < CZTB_MAX_SLOTS; ++k) o.code[k] = o.dom[k] = o.ord[k] = o.mult[k] = 0, o.radix[k] = 1;
    if (!sig) return -1;
    int black = 0, last = -1, run = 0;
    bool first = true;
    unsigned long long entries = 2;
    for (const char *p = sig;; ++p) {
        if (*p == '-' || *p == 0) {
            if (first) return *p == 0 && p == sig ? -1 : -2;   // an empty side
            if (*p == 0) { if (black != 1) return -1; break; }
            if (++black > 1) return -1;
            last = -1, run = 0, first = true;
            continue;
        }
        int l = 0;
        while (l < 7 && letters[l] != *p) ++l;
        if (l == 7) return -1;
        if (first && l != 0) return -2;
        first = false;
        if (l < last) return -3;
        run = l == last ? run + 1 : 1;
        if (run > most[l]) return -3;
        last = l;
        if (o.n == CZTB_MAX_SLOTS) return -4;
        o.code[o.n] = (uint8_t)(code[l] + 7 * black);
        o.dom[o.n] = (uint8_t)(dom[l] ? dom[l] + 4 * black : 0);
        o.radix[o.n] = (uint8_t)radix[l];
        o.ord[o.n] = (uint8_t)(run - 1);
        entries *= (unsigned long long)radix[l];
        if (entries > 0x7FFFFFFFull) return -4;
        ++o.n;
    }
    for (int k = 0; k < o.n; ++k)
        for (int j = 0; j < o.n; ++j) o.mult[k] = (uint8_t)(o.mult[k] + (o.code[j] == o.code[k]));
    o.entries = (uint32_t)entries;
    *d = o;
    return 0;
}
// the descriptor without slot j (never a king): the table a capture of that piece leads to
inline CztbDesc cztb_without(const CztbDesc &d, int j) {
    CztbDesc o = d;
    o.n = d.n - 1;
    o.entries = d.entries / d.radix[j];
    for (int k = 0; k < CZTB_MAX_SLOTS; ++k) {
        const int s = k < j ? k : k + 1;
        const bool in = s < d.n && k < o.n;
        o.code[k] = in ? d.code[s] : 0, o.dom[k] = in ? d.dom[s] : 0, o.radix[k] = in ? d.radix[s] : 1;
        o.ord[k] = in ? (uint8_t)(d.ord[s] - (d.code[s] == d.code[j] && s > j)) : 0;
        o.mult[k] = in ? (uint8_t)(d.mult[s] - (d.code[s] == d.code[j])) : 0;
    }
    return o;
}
// the signature string of a descriptor (buf: CZTB_MAX_SLOTS + 2 bytes)
inline void cztb_name(const CztbDesc &d, char *buf) {
    static const char by_code[] = "?KARBNPC";
    int at = 0;
    for (int k = 0; k < d.n; ++k) {
        if (k && d.code[k] == 8) buf[at++] = '-';
        buf[at++] = by_code[d.code[k] > 7 ? d.code[k] - 7 : d.code[k]];
    }
    buf[at] = 0;
}

// ---- domains: digit -> square, square -> digit (-1: the square is not in the domain); dom is wave-uniform ----------------------
CZM_FN int cztb_square(int dom, int dg) {
    const int black = dom > 4, kind = black ? dom - 4 : dom;
    if (kind == CZTB_DOM_K) return 9 * (dg / 3) + 3 + dg % 3 + (black ? 63 : 0);
    if (kind == CZTB_DOM_A) return (int)(((black ? 0x56544C4442ull : 0x17150D0503ull) >> (8 * dg)) & 0xFFu);   // 3 5 13 21 23 | 66 68 76 84 86
    if (kind == CZTB_DOM_B) return (int)(((black ? 0x575347433F332Full : 0x2A261A16120602ull) >> (8 * dg)) & 0xFFu);
    if (kind == CZTB_DOM_P) {   // red: files a c e g i of ranks 3, 4, then ranks 5 .. 9; black: ranks 0 .. 4, then files a c e g i of ranks 5, 6
        const int e = black ? dg - 45 : dg, part = 9 * (e / 5) + 2 * (e % 5);
        return black ? (dg < 45 ? dg : 45 + part) : (dg < 10 ? 27 + part : 35 + dg);
    }
    return dg;
}
CZM_FN int cztb_digit(int dom, int sq) {
    const int black = dom > 4, kind = black ? dom - 4 : dom;
    const int y = sq / 9, x = sq - 9 * y;
    if (kind == CZTB_DOM_K) {
        const int yy = black ? y - 7 : y;
        return (yy >= 0 && yy <= 2 && x >= 3 && x <= 5) ? 3 * yy + x - 3 : -1;
    }
    if (kind == CZTB_DOM_A || kind == CZTB_DOM_B) {   // the few squares, compared one by one
        int dg = -1;
#pragma unroll
        for (int k = 0; k < 7; ++k) dg = (k < (kind == CZTB_DOM_A ? 5 : 7) && cztb_square(dom, k) == sq) ? k : dg;
        return dg;
    }
    if (kind == CZTB_DOM_P) {
        const bool even = (x & 1) == 0;
        if (black) return sq < 45 ? sq : ((y <= 6 && even) ? 45 + 5 * (y - 5) + (x >> 1) : -1);
        return sq >= 45 ? sq - 35 : ((y >= 3 && even) ? 5 * (y - 3) + (x >> 1) : -1);
    }
    return sq;
}

// ---- index -> position ---------------------------------------------------------------------------------------------------------
// The squares and digits of the slots of `index` (< d.entries); returns the side to move.  *overlap: two slots share a square.
CZM_FN int cztb_unrank(const CztbDesc &d, uint32_t index, int (&sq)[CZTB_MAX_SLOTS], int (&dg)[CZTB_MAX_SLOTS], bool *overlap) {
    uint32_t m = index >> 1;
    uint64_t lo = 0ull, hi = 0ull;
    bool ov = false;
#pragma unroll
    for (int k = CZTB_MAX_SLOTS - 1; k >= 0; --k) {
        sq[k] = -1, dg[k] = 0;
        if (k < d.n) {
            const uint32_t r = d.radix[k], q = m / r;
            dg[k] = (int)(m - q * r);
            m = q;
            sq[k] = cztb_square(d.dom[k], dg[k]);
            const uint64_t bl = sq[k] < 64 ? 1ull << (sq[k] & 63) : 0ull, bh = sq[k] >= 64 ? 1ull << (sq[k] & 63) : 0ull;
            ov |= ((lo & bl) | (hi & bh)) != 0ull;
            lo |= bl, hi |= bh;
        }
    }
    *overlap = ov;
    return (int)(index & 1u);
}
// the slots' pieces on their squares as the 23 packed words of a board; put = false: an empty board
CZM_FN void cztb_words(const CztbDesc &d, const int (&sq)[CZTB_MAX_SLOTS], bool put, uint32_t (&w)[23]) {
#pragma unroll
    for (int i = 0; i < 23; ++i) w[i] = 0u;
#pragma unroll
    for (int k = 0; k < CZTB_MAX_SLOTS; ++k) {
        if (k < d.n) {
            const int q = put ? sq[k] : -4;
            const uint32_t v = (uint32_t)d.code[k] << (8 * (q & 3));
#pragma unroll
            for (int i = 0; i < 23; ++i) w[i] |= (q >> 2) == i ? v : 0u;
        }
    }
}

// ---- position -> index ---------------------------------------------------------------------------------------------------------
// The index of the position (w, side): among equal pieces the k-th in ascending square order stands on the k-th slot.
// Returns CZTB_MISS when the board's multiset of pieces is not the signature's (or a byte is no piece code), CZTB_ILLEGAL when
// a piece stands outside its domain (the position has no index), else 0 and *index.
// The four bit planes of a board's codes (czm_plane) and the OR of its bytes' high nibbles: what cztb_rank and
// cztb_material_key read of a position, taken once.
struct CztbPlanes {
    CzmSet p0, p1, p2, p3;
    uint32_t high;   // != 0: some byte is above 15
};
CZM_FN CztbPlanes cztb_planes(const uint32_t (&w)[23]) {
    uint32_t high = 0u;
#pragma unroll
    for (int i = 0; i < 23; ++i) high |= w[i] & 0xF0F0F0F0u;
    return CztbPlanes{czm_plane<0>(w), czm_plane<1>(w), czm_plane<2>(w), czm_plane<3>(w), high};
}
CZM_FN CzmSet cztb_occupied(const CztbPlanes &P) { return CzmSet{P.p0.lo | P.p1.lo | P.p2.lo | P.p3.lo, P.p0.hi | P.p1.hi | P.p2.hi | P.p3.hi}; }
// the squares whose byte is c (1 .. 15), given that no byte is above 15
CZM_FN CzmSet cztb_squares_of(const CztbPlanes &P, int c) {
    const CzmSet b0 = (c & 1) ? P.p0 : czm_not(P.p0), b1 = (c & 2) ? P.p1 : czm_not(P.p1), b2 = (c & 4) ? P.p2 : czm_not(P.p2), b3 = (c & 8) ? P.p3 : czm_not(P.p3);
    return czm_and(czm_and(b0, b1), czm_and(b2, b3));
}

CZM_FN int cztb_rank(const CztbDesc &d, const CztbPlanes &P, int side, uint32_t *index) {
    bool miss = P.high != 0u || czm_popcnt(cztb_occupied(P)) != d.n;
    bool outside = false;
    uint32_t m = 0u;
#pragma unroll
    for (int k = 0; k < CZTB_MAX_SLOTS; ++k) {
        if (k < d.n) {
            CzmSet s = cztb_squares_of(P, d.code[k]);   // d.code[k] is wave-uniform: the squares whose byte is that code
            miss |= czm_popcnt(s) != d.mult[k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r < d.ord[k]) s = czm_without(s, czm_lowest(s));
            const int q = czm_lowest(s), dg = cztb_digit(d.dom[k], q >= 0 ? q : 0);
            outside |= q < 0 || dg < 0;
            m = m * d.radix[k] + (uint32_t)(dg >= 0 ? dg : 0);
        }
    }
    *index = 2u * m + (uint32_t)(side ? 1 : 0);
    return miss ? CZTB_MISS : outside ? CZTB_ILLEGAL : 0;
}
CZM_FN int cztb_rank(const CztbDesc &d, const uint32_t (&w)[23], int side, uint32_t *index) { return cztb_rank(d, cztb_planes(w), side, index); }

// ---- the material key: which table a position belongs to --------------------------------------------------------------------------
// Sum over the piece codes c = 1 .. 14 of min(count of c, 7) << 3 c, and bit 45 when any byte is no piece code (15 and above):
// the key Tablebase.signatures_of (cchess_zero_amd/tablebase.py) groups boards by.  Two boards have one key iff they hold the same
// multiset of pieces (up to six of a kind), so a board whose key is a descriptor's is no CZTB_MISS of cztb_rank under it, and
// any other is.  A byte above 15 is counted under no code, as in the Python key: its square is taken out of the planes first —
// the rare path, a branch no board of a game takes.
#define CZTB_KEY_FOREIGN (1ull << 45)
CZM_FN uint64_t cztb_material_key(const CztbPlanes &P) {
    uint64_t key = (P.high != 0u || czm_popcnt(cztb_squares_of(P, 15)) != 0) ? CZTB_KEY_FOREIGN : 0ull;
#pragma unroll
    for (int c = 1; c <= 14; ++c) {
        const int n = czm_popcnt(cztb_squares_of(P, c));
        key += (uint64_t)(n < 7 ? n : 7) << (3 * c);
    }
    return key;
}
CZM_FN uint64_t cztb_material_key(const uint32_t (&w)[23]) {
    CztbPlanes P = cztb_planes(w);
    if (P.high != 0u) {   // the bytes above 15 become empty squares; the key keeps its bit 45
        uint32_t c[23];
#pragma unroll
        for (int i = 0; i < 23; ++i) {
            uint32_t h = w[i] & 0xF0F0F0F0u;
            h |= h >> 1, h |= h >> 2;
            c[i] = w[i] & ~(((h >> 4) & 0x01010101u) * 0xFFu);
        }
        const uint32_t high = P.high;
        P = cztb_planes(c);
        P.high = high;
    }
    return cztb_material_key(P);
}
// the key of every board of the descriptor's signature (host)
inline uint64_t cztb_desc_key(const CztbDesc &d) {
    uint64_t key = 0ull;
    for (int k = 0; k < d.n; ++k) key += 1ull << (3 * d.code[k]);   // at most five of a code: no field runs over
    return key;
}

// ---- a set of tables: the directory of keys (cz_tablebase_set.hip) -------------------------------------------------------------------
#define CZTB_SET_MAX 256   // CZ_TB_SET_MAX: the keys of a set fit 2 KB of LDS, and a closure has at most 2^8 signatures
// host: the directory order of n keys — order[i] = which of the keys given stands at place i, ascending by key, whatever order
// they came in.  -> 0; -1: n outside 1 .. CZTB_SET_MAX; 1 + i: the key at place i equals the one before it (a signature given
// twice: one key, one signature — the letters of a side have a fixed order)
inline int cztb_set_sort(int n, const uint64_t *keys, int *order) {
    if (n < 1 || n > CZTB_SET_MAX) return -1;
    for (int i = 0; i < n; ++i) {   // insertion: n is small
        int j = i;
        for (; j > 0 && keys[order[j - 1]] > keys[i]; --j) order[j] = order[j - 1];
        order[j] = i;
    }
    for (int i = 1; i < n; ++i)
        if (keys[order[i]] == keys[order[i - 1]]) return 1 + i;
    return 0;
}
// the place of `key` among the n sorted keys skeys[0 .. CZTB_SET_MAX) (~0 behind the last), -1 when it is none of them: eight
// steps, 128 + 64 + .. + 1, that count the keys below it — no step reads past index CZTB_SET_MAX - 2
CZM_FN int cztb_set_find(const uint64_t *skeys, int n, uint64_t key) {
    int lo = 0;
#pragma unroll
    for (int s = CZTB_SET_MAX / 2; s >= 1; s >>= 1) lo = skeys[lo + s - 1] < key ? lo + s : lo;
    return (lo < n && skeys[lo] == key) ? lo : -1;
}

// ---- one index's pass ------------------------------------------------------------------------------------------------------------
CZM_FN int cztb_plies(int v) { return (v < 0 ? -v : v) - 1; }
// is the child value u decided in fewer than `pass` plies (a draw of a finished table counts: it is neither won nor lost)
CZM_FN bool cztb_settled(int u, int pass) { return u != CZTB_UNKNOWN && u != CZTB_MISS && u != CZTB_ILLEGAL && cztb_plies(u) < pass; }

// Pass `pass` of index `index`, whose value is `cur`.  pass 0: the initialisation, every index -> CZTB_ILLEGAL (two slots share a
// square, czk_position refuses the board, or the mover can take the king), -1 (no king-safe move) or CZTB_UNKNOWN.  pass >= 1:
// an index that is CZTB_UNKNOWN walks its king-safe list; with u the value of a child,
//     some u < 0 settled below `pass`            -> min plies(u) + 2                  (a win)
//     else every u > 0 settled below `pass`      -> -(max plies(u) + 2)               (a loss)
//     else                                       -> CZTB_UNKNOWN
// and any other index keeps `cur`.  go = false (pass >= 1 and cur is not CZTB_UNKNOWN, or the lane has no index): the lane runs
// along on an EMPTY board, as in czg_step, so that the wave-wide loops wait for none of its pieces; it answers `cur`.
//   scr(i), put(k, label), mid(): czk_position's; get(k): label k of the list that put wrote (after a fence of the caller's
//   inside `listed`, called once when the list is complete);
//   read(t, i): the value at index i of table t, t = -1 this table, t = j the table without slot j (CZTB_UNKNOWN if there is none).
template <typename Scr, typename Put, typename Mid, typename Listed, typename Get, typename Read>
CZM_FN int cztb_step(const CztbDesc &d, uint32_t index, int cur, int pass, bool go, const CzmTables &T, const uint16_t *srcdst, Scr scr, Put put, Mid mid,
                     Listed listed, Get get, Read read) {
    int sq[CZTB_MAX_SLOTS], dg[CZTB_MAX_SLOTS];
    bool overlap;
    const int side = cztb_unrank(d, go ? index : 0u, sq, dg, &overlap);
    const bool board = go && !overlap;
    uint32_t w[23];
    cztb_words(d, sq, board, w);
    uint32_t pf = 0u;
    const int n = czk_position<true, false>(w, side, T, scr, put, [](int, uint32_t) {}, mid, &pf);
    listed();
    if (pass == 0) {
        if (!go) return cur;
        return (overlap || n < 0 || (pf & CZK_CAN_TAKE_KING)) ? CZTB_ILLEGAL : n == 0 ? -1 : CZTB_UNKNOWN;
    }
    const int nm = board && n > 0 ? n : 0;
    int win = 0x7FFF, lose = -1;   // the fewest plies of a lost child, the most of a won one
    bool all_won = true;
    for (int j = 0; CZM_ANY(j < nm); ++j) {
        const bool on = j < nm;
        const uint32_t label = on ? (uint32_t)get(j) : 0u;
        const uint32_t sd = on ? srcdst[label] : 0u;   // a listed label is < 2086
        const int from = (int)(sd & 0xFFu), to = (int)(sd >> 8);
        uint32_t m = 0u;
        int t = -1;
        bool ok = on;
#pragma unroll
        for (int k = 0; k < CZTB_MAX_SLOTS; ++k) {
            if (k < d.n) {
                const bool mover = sq[k] == from, taken = sq[k] == to;
                const int dt = cztb_digit(d.dom[k], to);
                ok &= !(mover && dt < 0);
                t = taken ? k : t;
                m = taken ? m : m * d.radix[k] + (uint32_t)(mover ? (dt >= 0 ? dt : 0) : dg[k]);
            }
        }
        const int u = ok ? read(t, 2u * m + (uint32_t)(1 - side)) : CZTB_UNKNOWN;
        const bool s = on && cztb_settled(u, pass);
        win = (s && u < 0 && cztb_plies(u) < win) ? cztb_plies(u) : win;
        lose = (s && u > 0 && cztb_plies(u) > lose) ? cztb_plies(u) : lose;
        all_won &= !on || (s && u > 0);
    }
    if (!go || cur != CZTB_UNKNOWN || nm == 0) return cur;
    return win != 0x7FFF ? win + 2 : all_won ? -(lose + 2) : CZTB_UNKNOWN;
}
