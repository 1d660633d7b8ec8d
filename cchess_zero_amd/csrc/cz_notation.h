// cz_notation.h — a move NAMED in WXF / Chinese notation, found in the position it is played in.  Such a move has no
// coordinates: "C2=5" is a piece kind, a file counted from the mover's right, a direction and a target file or a distance,
// and only the position says which squares that is.  cz_games_read (cz_notation.hip) therefore decodes inside the replay: the
// lane has its game's board and the ply's legal list at hand, czn_pick tries the token on every listed move and the ply is
// made when exactly one matches.  The reference has no such function (it never reads a game back).
// A token is one uint32.  Below 65536 it is a move label.  Otherwise four bytes, least significant first, b0 b1 b2 b3:
//   b0  the kind, one of K A E H R C P, or a file digit 1-9: the mover's PAWN on that file (b1 is then an ordinal)
//   b1  the source: a file digit 1-9, or an ordinal on the file: + frontmost, - rearmost, a-e the 1st .. 5th from the front
//   b2  + forward, - backward, = sideways
//   b3  a digit 1-9: the target file (=, and every move of H E A) or the distance (+ and - of R C P K)
// x = 0..8 are the files a..i, y = 0 is red's back rank; the file number of x is 9 - x for red and x + 1 for black; forward
// is +y for red and -y for black.  Bytes outside this alphabet match nothing, and so does b0 a digit with b1 a digit: no
// token value indexes anything.
// Host-compilable like cz_games.h (tests/notation_host.cpp compiles this very text).
#pragma once
#include "cz_games.h"

// the fields of a token.  kind: the piece code of the red piece of that kind (K 1, A 2, R 3, E 4, H 5, P 6, C 7), 0: a token
// that matches nothing; pfile: b0's file digit or 0; sfile: b1's file digit or 0; sord: 0 no ordinal, 1..5 for a..e, 6 for +,
// 7 for -; dir: +1 / -1 / 0 (=); d3: b3's digit
struct CznToken { int kind, pfile, sfile, sord, dir, d3; };

CZM_FN CznToken czn_token(uint32_t t) {
    const int b0 = (int)(t & 0xFFu), b1 = (int)((t >> 8) & 0xFFu), b2 = (int)((t >> 16) & 0xFFu), b3 = (int)(t >> 24);
    const bool d0 = b0 >= '1' && b0 <= '9';
    CznToken k;
    k.kind = b0 == 'K' ? 1 : b0 == 'A' ? 2 : b0 == 'R' ? 3 : b0 == 'E' ? 4 : b0 == 'H' ? 5 : (b0 == 'P' || d0) ? 6 : b0 == 'C' ? 7 : 0;
    k.pfile = d0 ? b0 - '0' : 0;
    k.sfile = (b1 >= '1' && b1 <= '9') ? b1 - '0' : 0;
    k.sord = b1 == '+' ? 6 : b1 == '-' ? 7 : (b1 >= 'a' && b1 <= 'e') ? b1 - 'a' + 1 : 0;
    k.dir = b2 == '+' ? 1 : b2 == '-' ? -1 : 0;
    k.d3 = (b3 >= '1' && b3 <= '9') ? b3 - '0' : 0;
    const bool ok = k.d3 != 0 && (b2 == '+' || b2 == '-' || b2 == '=') && (d0 ? k.sord != 0 : (k.sfile != 0 || k.sord != 0));
    k.kind = ok ? k.kind : 0;
    return k;
}

// The mover's pieces of the token's kind as a set of squares in FILE-major order, bit 10 x + y: ten consecutive bits are a file,
// so what an ordinal asks (how many of the kind stand on the file, how many of them in front) is a mask and two popcounts.  Built
// once per ply from the 23 words of the board before the move, bw(k), 0 <= k < 23, every square at a compile-time place: no
// board byte is read per listed move.  code: the piece code looked for (one that no square holds: the empty set).
struct CznSet { uint32_t w[3]; };
template <typename Bw>
CZM_FN CznSet czn_kind_set(uint32_t code, Bw bw) {
    CznSet s;
    s.w[0] = s.w[1] = s.w[2] = 0u;
#pragma unroll
    for (int k = 0; k < 23; ++k) {
        const uint32_t v = bw(k);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int q = 4 * k + b;
            if (q < 90) {
                const int bit = 10 * (q % 9) + q / 9;
                s.w[bit >> 5] |= ((v >> (8 * b)) & 0xFFu) == code ? 1u << (bit & 31) : 0u;
            }
        }
    }
    return s;
}

// Does the listed move from -> to of the side to move match the token?  S: czn_kind_set of the token's kind for the mover.
CZM_FN bool czn_match(const CznToken &k, int side, int from, int to, const CznSet &S) {
    const int fy = from / 9, fx = from - 9 * fy, ty = to / 9, tx = to - 9 * ty;
    const int ffile = side ? fx + 1 : 9 - fx, tfile = side ? tx + 1 : 9 - tx;
    const int dy = side ? fy - ty : ty - fy;   // forward is positive
    // the file of `from`: bits 10 fx .. 10 fx + 9 of the set, out of the pair of words they lie in
    const int lo = 10 * fx, wi = lo >> 5;
    const uint32_t p0 = wi == 0 ? S.w[0] : wi == 1 ? S.w[1] : S.w[2], p1 = wi == 0 ? S.w[1] : wi == 1 ? S.w[2] : 0u;
    const uint32_t col = (uint32_t)((((uint64_t)p1 << 32) | p0) >> (lo & 31)) & 0x3FFu;
    const bool own = (col >> fy) & 1u;         // the piece on `from` is of the kind
    const uint32_t front = side ? (1u << fy) - 1u : 0x3FFu & ~((2u << fy) - 1u);   // the squares of the file in front of `from`
    const int cnt = __builtin_popcount(col), ahead = __builtin_popcount(col & front), behind = cnt - 1 - ahead;
    const bool src = k.sord == 0 ? ffile == k.sfile : (cnt >= 2 && (k.sord == 6 ? ahead == 0 : k.sord == 7 ? behind == 0 : ahead == k.sord - 1));
    const bool leaper = k.kind == 2 || k.kind == 4 || k.kind == 5;   // A E H: the target file says where, = never
    const int ady = dy < 0 ? -dy : dy;
    const bool mv = k.dir == 0 ? (dy == 0 && tfile == k.d3 && !leaper)
                               : ((k.dir > 0 ? dy > 0 : dy < 0) && (leaper ? tfile == k.d3 : (tx == fx && ady == k.d3)));
    return k.kind != 0 && own && (k.pfile == 0 || ffile == k.pfile) && src && mv;
}

// czg_step_pick's hook for a token: a label token (< 65536) is left to the step's own search of the list; a text token is
// tried on the n listed moves: exactly one match -> label and idx are that move's; none -> CZG_ILLEGAL, more -> CZG_AMBIGUOUS.
//   text: this lane has a text token to decode (false: it runs along and nothing of it is changed);
//   list(j), j < 128: label number j of the list (read for j < n only);  sd(l), l < 2086: srcdst[l];  bw: as above.
// Four listed moves per trip of the wave-wide loop: their list and srcdst reads are independent of each other and in flight
// together, and nothing else of a candidate's test touches memory.
template <typename List, typename Sd, typename Bw>
CZM_FN int czn_pick(uint32_t tok, bool text, int side, int n, uint32_t &label, int &idx, List list, Sd sd, Bw bw) {
    int cnt = 0, at = -1;
    uint32_t lab = 0xFFFFu;
    if (CZM_ANY(text && n > 0)) {
        const CznToken k = czn_token(tok);
        const CznSet S = czn_kind_set(k.kind ? (uint32_t)(k.kind + (side ? 7 : 0)) : 0xFFu, bw);
        for (int j = 0; CZM_ANY(text && j < n); j += 4) {
            uint32_t l[4], s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) l[u] = (text && j + u < n) ? (uint32_t)list(j + u) : 0u;
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = sd(l[u] < 2086u ? l[u] : 0u);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool m = text && j + u < n && czn_match(k, side, (int)(s[u] & 0xFFu), (int)(s[u] >> 8), S);
                cnt += m ? 1 : 0;
                at = m ? j + u : at;
                lab = m ? l[u] : lab;
            }
        }
    }
    if (text) {
        idx = cnt == 1 ? at : -1;
        label = cnt == 1 ? lab : 0xFFFFu;
    }
    return cnt > 1 ? CZG_AMBIGUOUS : CZG_ILLEGAL;
}
