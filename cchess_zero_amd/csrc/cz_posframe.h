// cz_posframe.h — the frame of the lane-per-position rules kernels (k_movegen_mask, k_movegen_list in cz_rules.hip,
// k_movegen_kingsafe in cz_kingsafe.hip, k_threats in cz_chase.hip), once.  One lane owns one position: a wave walks groups of
// 64 positions with a stride, stages a group's 64 boards (5 760 contiguous bytes) in LDS, every lane pulls its own 90 bytes out
// as 23 dwords, the rules run in registers, and the results leave LDS as rows.  What a kernel keeps to itself is its LDS layout,
// its call into the rules and the order of its phases.  k_hash (cz_rules.hip) takes the fence, the board size and the launch
// helper from here and keeps its own loop (the reason stands there).  Device code, and the host's one launch helper.
#pragma once
#include "cz_internal.h"

#define CZF_BOARD_WORDS (64 * CZ_NSQ / 4)   /* a group's boards in LDS: 1 440 words; czf_unpack reads one word behind them */
#define CZF_LROW 65                         /* dwords per list row in LDS: 64 + 1 (the 64 lanes' 2-byte stores spread over the banks) */

// The fence between two phases that meet in LDS, for a workgroup that IS one wave or a region of LDS that only one wave
// touches.  A wave's LDS instructions execute in issue order, so all that is needed between the phases is that the LDS counter
// drains and that the compiler moves no memory operation across: a row that leaves through global stores has been read into
// registers (ds_read, in order) before a later phase writes the LDS under it, and the compiler's own waits cover the registers.
// Nothing needs the VECTOR-memory counter at zero: a __syncthreads() here waits for the prefetch just issued and for the
// previous rows' global stores as well (two exposed HBM round trips per group).
#define CZF_WAVE_FENCE() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// A launch of persistent waves (or workgroups): a chip's worth at the most, 256 CUs with per_cu resident on each.
inline int czf_persistent_grid(int ngroups, int per_cu) { return ngroups < 256 * per_cu ? ngroups : 256 * per_cu; }

// Group grp of a batch of G positions: its first position, its size (64, less in a batch's last group) and whether the lane
// owns one.  A wave walks `for (grp = wave; grp < czf_ngroups(G); grp += nwaves)`, the caller numbering its waves.
struct CzfGroup {
    int g0, np;
    bool live;
};
__device__ inline int czf_ngroups(int G) { return (G + 63) >> 6; }
__device__ inline CzfGroup czf_group(int grp, int G, int lane) {
    const int g0 = grp * 64, np = min(64, G - g0);
    return {g0, np, lane < np};
}

// The board loader.  A wave requests the NEXT group's 5 760 board bytes (six 16-byte loads per lane) and side bytes into
// registers before it computes the current one, so that the only HBM round trip a wave waits for is its first (SQ counters of
// a one-group-per-wave kernel: half of a wave's life in s_waitcnt).  That needs 16-byte aligned boards (g0 * 90 is a multiple
// of 16); other addresses take the byte path without it, the side byte read in place.
struct CzfLoader {
    const uint8_t *boards, *side;
    int G, lane;
    bool al16;
    uint4 pre[6];
    int presd;

    __device__ CzfLoader(const uint8_t *boards_, const uint8_t *side_, int G_, int lane_)
        : boards(boards_), side(side_), G(G_), lane(lane_), al16((reinterpret_cast<uintptr_t>(boards_) & 15u) == 0), presd(0) {}

    // asks for group grp, if there is one: in flight until stage()
    __device__ void request(int grp) {
        if (!al16 || grp >= czf_ngroups(G)) return;
        const CzfGroup g = czf_group(grp, G, lane);
        const int nbytes = g.np * CZ_NSQ;
        const uint8_t *src = boards + (size_t)g.g0 * CZ_NSQ;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int i = lane + 64 * k;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (i * 16 + 16 <= nbytes) v = reinterpret_cast<const uint4 *>(src)[i];   // the ragged piece of a batch's last group: stage()
            pre[k] = v;
        }
        presd = (g.live && side[g.g0 + lane]) ? 1 : 0;
    }

    // group g (the one last requested) -> rows[0 .. CZF_BOARD_WORDS); returns the lane's side to move (0 for a dead lane)
    __device__ int stage(uint32_t *rows, const CzfGroup &g) const {
        const uint8_t *src = boards + (size_t)g.g0 * CZ_NSQ;
        uint8_t *dst = reinterpret_cast<uint8_t *>(rows);
        const int nbytes = g.np * CZ_NSQ;
        if (!al16) {
            for (int i = lane; i < nbytes; i += 64) dst[i] = src[i];
            return (g.live && side[g.g0 + lane]) ? 1 : 0;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (lane + 64 * k < CZF_BOARD_WORDS / 4) reinterpret_cast<uint4 *>(rows)[lane + 64 * k] = pre[k];
        if (g.np < 64) {   // the last group of a batch: its ragged 16-byte piece byte by byte, never past the batch (wave-uniform branch)
            const int full = nbytes & ~15;
            if (lane < nbytes - full) dst[full + lane] = src[full + lane];
        }
        return presd;
    }
};

// The lane's board out of the staged rows: its 90 bytes start at byte 90 * lane, 4-aligned for even lanes, 2 (mod 4) for odd
// ones (funnel shift; lane 63 reads word CZF_BOARD_WORDS, which rows must hold).  A dead lane gets an empty board.
__device__ inline void czf_unpack(const uint32_t *rows, int lane, bool live, uint32_t (&w)[23]) {
    const int b0 = (CZ_NSQ * lane) >> 2, sh = (lane & 1) * 16;
    uint32_t d[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) d[k] = rows[b0 + k];
#pragma unroll
    for (int k = 0; k < 23; ++k) w[k] = __builtin_amdgcn_alignbit(d[k + 1], d[k], (uint32_t)sh);
    w[22] &= 0x0000FFFFu;
    if (!live) {
#pragma unroll
        for (int k = 0; k < 23; ++k) w[k] = 0u;
    }
}

// nrows (<= FULL) mask rows of CZ_MASK_WORDS words, contiguous in LDS as in the ABI, to global memory: FULL rows as statically
// counted 16-byte stores (the waits on a prefetch in flight stay counted too), a ragged last group in 16-byte pieces and a
// dword tail, a destination that is not 16-byte aligned in dwords.  FULL rows are a whole number of 16-byte pieces.
template <int FULL>
__device__ inline void czf_store_mask_rows(uint32_t *__restrict__ dstm, const uint32_t *rows, int nrows, int lane) {
    constexpr int PIECES = FULL * CZ_MASK_WORDS / 4;
    static_assert(FULL * CZ_MASK_WORDS % 4 == 0, "FULL rows end on a 16-byte piece");
    const bool al16 = (reinterpret_cast<uintptr_t>(dstm) & 15u) == 0;
    if (al16 && nrows == FULL) {
#pragma unroll
        for (int k = 0; k < PIECES / 64; ++k) reinterpret_cast<uint4 *>(dstm)[lane + 64 * k] = reinterpret_cast<const uint4 *>(rows)[lane + 64 * k];
        if (lane < PIECES % 64) reinterpret_cast<uint4 *>(dstm)[lane + PIECES / 64 * 64] = reinterpret_cast<const uint4 *>(rows)[lane + PIECES / 64 * 64];
    } else if (al16) {
        const int nw = nrows * CZ_MASK_WORDS;
        for (int i = lane; i < nw / 4; i += 64) reinterpret_cast<uint4 *>(dstm)[i] = reinterpret_cast<const uint4 *>(rows)[i];
        if (lane < (nw & 3)) dstm[(nw & ~3) + lane] = rows[(nw & ~3) + lane];   // fewer than four words behind the last piece
    } else {
        for (int i = lane; i < nrows * CZ_MASK_WORDS; i += 64) dstm[i] = rows[i];
    }
}

// The group's list rows (CZF_LROW words apart in LDS) to moves (16-byte aligned): 64 rows of sixteen 16-byte pieces, a row up
// to 128 labels with the padding, else up to the count n of the lane that owns it (the labels behind it in its last piece are
// undefined; a refused position, n < 0, writes nothing).
__device__ inline void czf_store_list_rows(uint16_t *__restrict__ moves, const uint32_t *rows, const CzfGroup &g, int n, bool pad, int lane) {
    uint4 *dst = reinterpret_cast<uint4 *>(moves + (size_t)g.g0 * CZD_MAXMOVES);
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int idx = lane + 64 * k, pp = idx >> 4, j = idx & 15;
        const int npp = pad ? 128 : __shfl(n, pp, 64);
        if (pp < g.np && 8 * j < npp) {
            const uint32_t *src = rows + pp * CZF_LROW + 4 * j;
            dst[idx] = make_uint4(src[0], src[1], src[2], src[3]);
        }
    }
}
