// cz_successors.hip — cz_successors: every successor position of G positions, driven by a move list (cz_movegen's,
// cz_movegen_ex's or cz_movegen_kingsafe's) and the exclusive prefix sum of its counts.  Child offsets[g] + j is parent g after
// moves[g][j]; the order of the output is a function of the input alone (no atomics, no cursor).
// The kernel is store-bound (a parent's 90 bytes in, ~40 x 90 bytes out) and is laid out around its stores, in the frame of
// cz_posframe.h: a wave owns a group of 64 parents, stages their boards in LDS (the next group's prefetched) and walks the
// group's children, one contiguous byte range [90 offsets[g0], 90 offsets[g0 + np]) of out_boards, in TILES of 5 120 bytes that
// start on 16-byte lines of the output.  Per tile: one lane = one child that touches it (58 at the most) — the lane finds its
// parent in the group's 64 offsets (six LDS reads), pulls the parent's 23 dwords out of the staged boards with the funnel shift
// that lands them on the CHILD's dword phase in the tile, writes them as dwords (its two ragged ends as halfwords: they share a
// dword with the neighbouring child, another lane), and patches the two squares of its move as bytes.  Then the tile leaves as
// 16-byte pieces, five instructions of 64 consecutive pieces: every store instruction is a contiguous kilobyte.  A child that
// straddles two tiles is built in both (the tile has 96 bytes of slack on either side, so nothing is bounds-checked while it is
// built) and writes its side / captured / parent / label in the tile that holds its first byte.
// THE BOUNDARY: a group's range starts and ends on even bytes, not on 16-byte lines, and the piece at either end is shared with
// the neighbouring group — another wave.  Those two pieces leave as 2-byte stores of the bytes inside the range only (lanes
// 0 .. 7 the head piece, 8 .. 15 the tail piece); no byte outside [90 offsets[g0], 90 offsets[g0 + np]) is ever written, none
// of a neighbour's is read.  The labels of the NEXT tile are requested before the current one is built, so the only exposed
// round trips are a group's first.  offsets are clamped into [0, total] and a list index into 0 .. 127: whatever the offsets
// hold, no access leaves the arrays.
#include "cz_internal.h"
#include "cz_posframe.h"

namespace {

constexpr int CZS_TILE = 5120;    // bytes of out_boards per tile: 320 pieces, five per lane
constexpr int CZS_SLACK = 96;     // bytes before and behind the tile in LDS: a straddling child is written whole (> 90, a multiple of 16)
constexpr int CZS_PAD = 4;        // words before and behind the staged boards: the funnel shift reads one word before / behind a board

struct CzsChild {   // one lane's child of one tile
    int cr, d, pp;  // the child's index inside the group's range, its first byte relative to the tile (-88 .. CZS_TILE - 2), its parent's lane
    bool ok;
    uint16_t label;
};

__global__ __launch_bounds__(64) void k_successors(const uint16_t *__restrict__ srcdst, const uint8_t *__restrict__ boards,
                                                   const uint8_t *__restrict__ side, int G, const uint16_t *__restrict__ moves,
                                                   const int32_t *__restrict__ offsets, int total, uint8_t *__restrict__ out_boards,
                                                   uint8_t *__restrict__ out_side, uint8_t *__restrict__ out_captured,
                                                   int32_t *__restrict__ out_parent, uint16_t *__restrict__ out_label) {
    __shared__ __attribute__((aligned(16))) uint32_t brd[CZS_PAD + CZF_BOARD_WORDS + CZS_PAD];
    __shared__ __attribute__((aligned(16))) uint32_t tile[(CZS_SLACK + CZS_TILE + CZS_SLACK) / 4];
    __shared__ int offl[64];                    // the group's offsets relative to its first child; INT_MAX behind the last parent
    __shared__ uint16_t sdt[CZ_NLABELS + 2];   // label -> src | dst << 8
    const int lane = threadIdx.x;
    for (int i = lane; i < CZ_NLABELS; i += 64) sdt[i] = srcdst[i];
    const uint8_t *const brd8 = reinterpret_cast<const uint8_t *>(brd + CZS_PAD);
    uint8_t *const tile8 = reinterpret_cast<uint8_t *>(tile);
    uint16_t *const tile16 = reinterpret_cast<uint16_t *>(tile);
    CzfLoader ld(boards, side, G, lane);
    ld.request(blockIdx.x);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        const int c0 = __builtin_amdgcn_readfirstlane(min(max(offsets[g.g0], 0), total));                // wave-uniform: in scalar registers
        const int c1 = __builtin_amdgcn_readfirstlane(min(max(offsets[g.g0 + g.np], c0), total));
        const int om = g.live ? min(max(offsets[g.g0 + lane], c0), c1) - c0 : 0x7FFFFFFF;
        const int nch = c1 - c0;
        CZF_WAVE_FENCE();   // the previous group's last tile has left (and the table is in place)
        const int sd = ld.stage(brd + CZS_PAD, g);
        offl[lane] = om;
        ld.request(grp + gridDim.x);   // in flight while this group's children are written
        CZF_WAVE_FENCE();
        if (nch == 0) continue;        // wave-uniform
        const long long gb = 90ll * c0;
        const int rel0 = (int)(gb & 15);                     // the range's first byte inside its 16-byte line
        uint8_t *const wbase = out_boards + (gb - rel0);    // 16-byte aligned: the tiles count from here
        const int rel_end = rel0 + CZ_NSQ * nch;             // <= 16 + 90 * 8192
        const int ntiles = (rel_end + CZS_TILE - 1) / CZS_TILE;

        // the lane's child of tile t: children whose first byte lies in (t * CZS_TILE - 90, (t + 1) * CZS_TILE), in order
        auto prep = [&](int t) -> CzsChild {
            CzsChild c;
            const int tb = t * CZS_TILE;
            c.cr = (t ? (tb - rel0) / CZ_NSQ : 0) + lane;
            c.d = rel0 + CZ_NSQ * c.cr - tb;
            c.ok = c.cr < nch && c.d < CZS_TILE;
            int pp = 0;   // the last parent whose offset is <= cr: the one with offl[pp] <= cr < offl[pp + 1]
#pragma unroll
            for (int s = 32; s; s >>= 1)
                if (offl[pp + s] <= c.cr) pp += s;   // pp + s <= 63
            c.pp = c.ok ? pp : 0;
            c.label = 0xFFFF;
            if (c.ok) c.label = moves[(size_t)(g.g0 + c.pp) * CZD_MAXMOVES + ((c.cr - offl[c.pp]) & (CZD_MAXMOVES - 1))];
            return c;
        };

        CzsChild nx = prep(0);
        for (int t = 0; t < ntiles; ++t) {
            const CzsChild cur = nx;
            nx = prep(t + 1);   // its labels are in flight while this tile is built and stored (behind the last tile no lane is ok)
            const int psd = __shfl(sd, cur.pp, 64);
            if (cur.ok) {
                const int pp = cur.pp, off = CZS_SLACK + cur.d;   // the child's first byte in the tile's LDS: even, > 0
                const int D = off >> 2, hd = (off >> 1) & 1, delta = (pp & 1) - hd;
                // halfword h of the child is halfword (pp & 1) + h behind word b0 of the staged boards and halfword hd + h behind word D
                // of the tile: word m of the child's 23 in the tile starts `delta` halfwords behind word b0 + m
                const uint32_t *src = brd + CZS_PAD + ((CZ_NSQ * pp) >> 2) - (delta < 0 ? 1 : 0);
                const uint32_t sh = delta ? 16u : 0u;
                uint32_t e[24], u[23];
#pragma unroll
                for (int k = 0; k < 24; ++k) e[k] = src[k];
#pragma unroll
                for (int k = 0; k < 23; ++k) u[k] = __builtin_amdgcn_alignbit(e[k + 1], e[k], sh);
                // hd = 0: words 0 .. 21 and the low half of word 22; hd = 1: the high half of word 0 and words 1 .. 22.  The other
                // half of an end word is the neighbouring child's.
                if (hd) tile16[2 * D + 1] = (uint16_t)(u[0] >> 16);
                else tile[D] = u[0];
#pragma unroll
                for (int k = 1; k < 22; ++k) tile[D + k] = u[k];
                if (hd) tile[D + 22] = u[22];
                else tile16[2 * (D + 22)] = (uint16_t)u[22];
                uint8_t cap = 0;
                if (cur.label < CZ_NLABELS) {   // sim_do_action, as k_apply_move; any other label leaves the parent's board
                    const int sq = sdt[cur.label], from = sq & 0xFF, to = sq >> 8;
                    const uint8_t pc = brd8[CZ_NSQ * pp + from];
                    cap = brd8[CZ_NSQ * pp + to];
                    tile8[off + from] = 0;
                    tile8[off + to] = pc;
                }
                if (cur.d >= 0) {   // the tile that holds the child's first byte
                    const size_t c = (size_t)c0 + cur.cr;
                    if (out_side) out_side[c] = psd ? 0 : 1;
                    if (out_captured) out_captured[c] = cap;
                    if (out_parent) out_parent[c] = g.g0 + pp;
                    if (out_label) out_label[c] = cur.label;
                }
            }
            CZF_WAVE_FENCE();   // the tile is built
            const int tb = t * CZS_TILE;
            const int lo = max(rel0 - tb, 0), hi = min(rel_end - tb, CZS_TILE);   // the range inside this tile
            uint8_t *const dst = wbase + tb;
#pragma unroll
            for (int k = 0; k < CZS_TILE / 16 / 64; ++k) {
                const int p = lane + 64 * k;
                if (16 * p >= lo && 16 * p + 16 <= hi) reinterpret_cast<uint4 *>(dst)[p] = reinterpret_cast<const uint4 *>(tile)[CZS_SLACK / 16 + p];
            }
            // the range's two ragged pieces (the head in a group's first tile, the tail in its last): the bytes inside it, two at a time
            if (((lo | hi) & 15) && lane < 16) {
                const bool head = lane < 8;
                const int piece = head ? lo >> 4 : hi >> 4;
                const int o = 16 * piece + 2 * (lane & 7);
                const bool ragged = head ? (lo & 15) != 0 : ((hi & 15) != 0 && !((lo & 15) && (hi >> 4) == (lo >> 4)));
                if (ragged && o >= lo && o < hi) reinterpret_cast<uint16_t *>(dst)[o >> 1] = tile16[(CZS_SLACK + o) >> 1];
            }
            CZF_WAVE_FENCE();   // the tile is in registers on its way out
        }
    }
}

}  // namespace

int cz_successors(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, const uint16_t *moves, const int32_t *offsets, int total,
                  uint8_t *out_boards, uint8_t *out_side, uint8_t *out_captured, int32_t *out_parent, uint16_t *out_label) {
    CZ_REQUIRE(c && G >= 0 && total >= 0, "cz_successors: null ctx / negative G or total");
    if (G == 0 || total == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && moves && offsets && out_boards, "cz_successors: boards, side, moves, offsets, out_boards required");
    if (reinterpret_cast<uintptr_t>(out_boards) & 15u) { cz_set_error("cz_successors: out_boards must be 16-byte aligned"); return CZ_EINVAL; }
    const dim3 grid(czf_persistent_grid((G + 63) / 64, 10));   // 15.5 KB of LDS per wave: ten waves per CU
    hipLaunchKernelGGL(k_successors, grid, dim3(64), 0, c->stream, c->tab.srcdst, boards, side, G, moves, offsets, total, out_boards, out_side,
                       out_captured, out_parent, out_label);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
