// tests/perft_host.cpp — a recursive perft on the HOST over the library's king-safe move generator (czk_position,
// cchess_zero_amd/csrc/cz_kingsafe.h, the function cz_movegen_kingsafe runs one lane per position), so that the published
// Xiangqi perft table can anchor that definition without a GPU: tests/golden/gen_perft.py writes tests/golden/perft.json with
// it, tests/test_perft_cpu.py holds it to the fixture.  Test infrastructure: nothing in the product path uses it.
#include <string.h>
#include "../cchess_zero_amd/csrc/cz_kingsafe.h"

namespace {

struct Perft {
    const CzmTables *t;
    const uint16_t *srcdst;   // label -> src | dst << 8
    int depth, stats;
    long long *nodes, *captures, *checks, *mates;   // [depth + 1]
    int refused;
};

// the position's king-safe list (list != NULL) or its count alone -> count, -1 when the generator refuses the board
int generate(const Perft &p, const uint8_t *board, int side, uint16_t *list, uint32_t *pf) {
    uint32_t w[23], scratch[CZK_SCRATCH];
    unsigned char buf[92];
    memcpy(buf, board, 90);
    buf[90] = buf[91] = 0;
    memcpy(w, buf, 92);
    auto scr = [&scratch](int k) -> uint32_t & { return scratch[k]; };
    *pf = 0;
    if (!list) return czk_position<false, false>(w, side, *p.t, scr, [](int, int) {}, [](int, uint32_t) {}, [] {}, pf);
    return czk_position<true, false>(w, side, *p.t, scr, [list](int k, int label) { list[k & 127] = (uint16_t)label; }, [](int, uint32_t) {}, [] {}, pf);
}

// the position `board` of depth d, reached by a move that took `captured`
void walk(Perft &p, uint8_t *board, int side, int d, int captured) {
    p.nodes[d] += 1;
    if (captured) p.captures[d] += 1;
    if (d == p.depth && !p.stats) return;
    uint16_t list[128];
    uint32_t pf;
    const int n = generate(p, board, side, d == p.depth ? nullptr : list, &pf);
    if (n < 0) { p.refused = 1; return; }
    if (p.stats) {
        if (pf & CZK_IN_CHECK) p.checks[d] += 1;
        if (pf & CZK_NO_SAFE_MOVE) p.mates[d] += 1;
    }
    if (d == p.depth) return;
    if (!p.stats && d == p.depth - 1) { p.nodes[p.depth] += n; return; }   // the last ply counted, not made
    for (int j = 0; j < n; ++j) {
        const int from = p.srcdst[list[j]] & 0xFF, to = p.srcdst[list[j]] >> 8;
        const uint8_t pc = board[from], cap = board[to];
        board[to] = pc;
        board[from] = 0;
        walk(p, board, side ^ 1, d + 1, cap);
        board[from] = pc;
        board[to] = cap;
    }
}

}  // namespace

extern "C" void perft_host_tables(const int16_t *lut, CzmTables *t) { czm_build_tables(lut, t); }
extern "C" int perft_host_sizeof_tables(void) { return (int)sizeof(CzmTables); }
// board [90], side -> nodes / captures / checks / mates [depth + 1] (column 0 the root; without stats only nodes are written, the
// last ply counted from its parents' lists); returns 0, or -1 when a position on the way is one the generator refuses
extern "C" int perft_host(const CzmTables *t, const uint16_t *srcdst, const uint8_t *board, int side, int depth, int stats, long long *nodes,
                          long long *captures, long long *checks, long long *mates) {
    Perft p{t, srcdst, depth, stats, nodes, captures, checks, mates, 0};
    for (int d = 0; d <= depth; ++d) nodes[d] = captures[d] = checks[d] = mates[d] = 0;
    uint8_t b[90];
    memcpy(b, board, 90);
    walk(p, b, side ? 1 : 0, 0, 0);
    return p.refused ? -1 : 0;
}
