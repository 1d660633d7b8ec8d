// cz_book.hip — the opening book's kernels and their host entry points (include/cchess_hip.h: BOOK): cz_book_keys, cz_book_entries,
// cz_book_probe, cz_book_choose.  A book is a sorted table (key, label) -> games, wins, draws built from recorded games
// (cchess_zero_amd/book.py); the arrays are the caller's, there is no handle.
// All kernels are in the frame of cz_posframe.h, like k_tb_probe_set: one lane per position, one wave per group of 64, persistent,
// the boards staged through LDS with the next group requested before the current one is computed (k_book_entries takes the ROWS
// path: every lane loads the head of its own 608-byte record), CZF_WAVE_FENCE between the phases.
// THE CANONICAL KEY.  k is cz_hash's key, k' the key of the board with its files reversed; both come from the lane's 23 dwords
// in one pass: square q = 9 r + f adds Z[c][q] to k and Z[c][q + 8 - 2 f] to k', both offsets compile-time constants of the
// unrolled loop, so the pair is one two-address LDS read behind one row address and no mirrored board exists anywhere.
// LDS: the Zobrist table as in k_hash, 16 x 90 keys of 8 bytes (row 0 and row 15 behind the side key are zero: an empty square
// and a byte above 14 need no branch), shared by the FOUR waves of a workgroup (k_hash's comment in cz_rules.hip: one table per
// wave leaves 9 waves per CU).  A row is 720 bytes = 180 dwords, 180 = 52 (mod 64): the fifteen rows' bank offsets 52 c mod 64
// are fifteen different multiples of 4, so at one square lanes with different pieces read different bank pairs and lanes with
// the same piece read the same address (a broadcast): the ds_read_b64 pairs are conflict-free.  With the four staging areas
// 34.6 KB per workgroup; k_book_entries stages nothing (11.5 KB).
// OCCUPANCY is set by registers, not LDS: the compiler keeps most of the 180 LDS reads of a position in flight at once and the
// staged kernels take about 220 VGPRs (2 waves per SIMD, 2 workgroups per CU).  Asking for 3 or 4 waves per SIMD through
// __launch_bounds__ makes it spill 50-90 registers to scratch rather than shorten the read queue, and scheduling barriers in the
// key loop raised the count; the kernels are left at what compiles without scratch (tests/test_book_host_cpu.py checks that).
// No scratch, no register array indexed at run time, no atomics; one __syncthreads (the table) per workgroup.
#include "cz_internal.h"
#include "cz_posframe.h"

#define CZB_WAVES 4
#define CZB_SKIPPED 255

namespace {

// the table into LDS, by the whole workgroup (the caller synchronises)
__device__ inline void czb_load_zobrist(uint64_t *Z, const uint64_t *__restrict__ zob) {
    for (int i = threadIdx.x; i < 16 * CZ_NSQ; i += 64 * CZB_WAVES) Z[i] = i <= 15 * CZ_NSQ ? zob[i] : 0ull;
}

struct CzbKey {
    uint64_t key;   // min(k, k') as unsigned
    int mir;        // 0: k < k', 1: mirrored (k' < k), 2: self-mirror
};

__device__ inline CzbKey czb_key(const uint32_t (&w)[23], int sd, const uint64_t *Z) {
    uint64_t h = sd ? Z[15 * CZ_NSQ] : 0ull, hm = h;
#pragma unroll
    for (int k = 0; k < 23; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = 4 * k + j;
            if (q < CZ_NSQ) {
                const uint32_t c = (w[k] >> (8 * j)) & 0xFFu;
                const uint64_t *row = Z + (c < 15u ? c : 0u) * CZ_NSQ;
                h ^= row[q];
                hm ^= row[q + 8 - 2 * (q % 9)];
            }
        }
    }
    return {hm < h ? hm : h, hm < h ? 1 : hm == h ? 2 : 0};
}

// the first entry of `key` among bkey[0 .. E) ascending, and how many there are: (-1, 0) for none
__device__ inline void czb_find(const uint64_t *__restrict__ bkey, int E, uint64_t key, int &first, int &count) {
    int lo = 0, hi = E;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (bkey[mid] < key) lo = mid + 1; else hi = mid;
    }
    int ub = lo;
    hi = E;
    while (ub < hi) {
        const int mid = ub + ((hi - ub) >> 1);
        if (bkey[mid] <= key) ub = mid + 1; else hi = mid;
    }
    count = ub - lo;
    first = count ? lo : -1;
}

// the frame's staged loop, once: body(g, w, sd) per group with the lane's board in w.  rows: the wave's own staging area.
template <typename Body>
__device__ inline void czb_walk(const uint8_t *__restrict__ boards, const uint8_t *__restrict__ side, int G, uint32_t *rows, Body body) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nwaves = gridDim.x * CZB_WAVES, w0 = blockIdx.x * CZB_WAVES + wv;
    CzfLoader ld(boards, side, G, lane);
    ld.request(w0);
    for (int grp = w0; grp < czf_ngroups(G); grp += nwaves) {
        const CzfGroup g = czf_group(grp, G, lane);
        CZF_WAVE_FENCE();   // the previous group's boards are in registers
        const int sd = ld.stage(rows, g);
        CZF_WAVE_FENCE();
        uint32_t w[23];
        czf_unpack(rows, lane, g.live, w);
        ld.request(grp + nwaves);   // in flight while this group is computed
        body(g, w, sd);
    }
}

__global__ __launch_bounds__(64 * CZB_WAVES) void k_book_keys(CzTables tab, const uint8_t *__restrict__ boards, const uint8_t *__restrict__ side, int G,
                                                              uint64_t *__restrict__ key, uint8_t *__restrict__ mirrored) {
    __shared__ __attribute__((aligned(16))) uint32_t rows_all[CZB_WAVES][CZF_BOARD_WORDS + 4];
    __shared__ uint64_t Z[16 * CZ_NSQ];
    czb_load_zobrist(Z, tab.zob);
    __syncthreads();   // the only workgroup-wide one: from here on every wave walks its own groups
    const int lane = threadIdx.x & 63;
    czb_walk(boards, side, G, rows_all[threadIdx.x >> 6], [&](const CzfGroup &g, const uint32_t (&w)[23], int sd) {
        const CzbKey k = czb_key(w, sd, Z);
        if (g.live) {
            key[g.g0 + lane] = k.key;
            if (mirrored) mirrored[g.g0 + lane] = (uint8_t)k.mir;
        }
    });
}

// The ROWS path: lane = record.  The first 96 bytes of a record are the board and, in the last 16-byte piece, side, count, z,
// flags and ply; the 128 visits follow at CZ_REC_VISITS as sixteen 16-byte pieces, of which the first ceil(count / 8) are read.
__global__ __launch_bounds__(64 * CZB_WAVES) void k_book_entries(CzTables tab, const int16_t *__restrict__ mirror, const uint8_t *__restrict__ records, int n,
                                                                 int max_ply, uint64_t *__restrict__ key, uint16_t *__restrict__ label,
                                                                 uint8_t *__restrict__ outcome) {
    static_assert(CZ_REC_SIDE == 90 && CZ_REC_COUNT == 91 && CZ_REC_Z == 92 && CZ_REC_PLY == 94 && CZ_REC_BYTES % 16 == 0 && CZ_REC_VISITS % 16 == 0,
                  "the record's head is read as six 16-byte pieces");
    __shared__ uint64_t Z[16 * CZ_NSQ];
    czb_load_zobrist(Z, tab.zob);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nwaves = gridDim.x * CZB_WAVES, w0 = blockIdx.x * CZB_WAVES + wv;
    for (int grp = w0; grp < czf_ngroups(n); grp += nwaves) {
        const CzfGroup g = czf_group(grp, n, lane);
        if (!g.live) continue;
        const uint8_t *rec = records + (size_t)(g.g0 + lane) * CZ_REC_BYTES;
        uint4 v[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] = reinterpret_cast<const uint4 *>(rec)[k];
        uint32_t w[23];
#pragma unroll
        for (int k = 0; k < 23; ++k) w[k] = (k & 3) == 0 ? v[k >> 2].x : (k & 3) == 1 ? v[k >> 2].y : (k & 3) == 2 ? v[k >> 2].z : v[k >> 2].w;
        const int sd = ((w[22] >> 16) & 0xFFu) ? 1 : 0, count = min((int)(w[22] >> 24), CZD_MAXMOVES);
        const int z = (int)(int8_t)(v[5].w & 0xFFu), ply = (int)(v[5].w >> 16);
        w[22] &= 0x0000FFFFu;
        const CzbKey k = czb_key(w, sd, Z);
        uint32_t lab = 0xFFFFu, out = CZB_SKIPPED;
        if (count > 0 && !(max_ply > 0 && ply >= max_ply)) {
            int best = -1, at = 0;   // the FIRST maximum of the first `count` visits
            for (int p = 0; 8 * p < count; ++p) {
                const uint4 x = reinterpret_cast<const uint4 *>(rec + CZ_REC_VISITS)[p];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t d = j < 2 ? x.x : j < 4 ? x.y : j < 6 ? x.z : x.w;
                    const int vis = (int)((d >> (16 * (j & 1))) & 0xFFFFu);
                    if (8 * p + j < count && vis > best) best = vis, at = 8 * p + j;
                }
            }
            lab = reinterpret_cast<const uint16_t *>(rec + CZ_REC_LABELS)[at];
            if (lab < (uint32_t)CZ_NLABELS) {
                const uint32_t ml = (uint32_t)(uint16_t)mirror[lab];
                lab = k.mir == 1 ? ml : k.mir == 2 ? min(lab, ml) : lab;
            }
            out = z > 0 ? 0u : z == 0 ? 1u : 2u;
        }
        key[g.g0 + lane] = k.key;
        label[g.g0 + lane] = (uint16_t)lab;
        outcome[g.g0 + lane] = (uint8_t)out;
    }
}

// CHOOSE false: cz_book_probe.  true: cz_book_choose, the pick among the found entries in the same lane.
template <bool CHOOSE>
__global__ __launch_bounds__(64 * CZB_WAVES) void k_book_probe(CzTables tab, const int16_t *__restrict__ mirror, int E, const uint64_t *__restrict__ bkey,
                                                               const uint16_t *__restrict__ blabel, const uint32_t *__restrict__ bgames,
                                                               const uint8_t *__restrict__ boards, const uint8_t *__restrict__ side,
                                                               const uint32_t *__restrict__ allowed, int G, uint32_t min_games, int mode,
                                                               const uint32_t *__restrict__ rnd, int32_t *__restrict__ first, int32_t *__restrict__ count,
                                                               uint8_t *__restrict__ mirrored, uint16_t *__restrict__ played, int32_t *__restrict__ index) {
    __shared__ __attribute__((aligned(16))) uint32_t rows_all[CZB_WAVES][CZF_BOARD_WORDS + 4];
    __shared__ uint64_t Z[16 * CZ_NSQ];
    czb_load_zobrist(Z, tab.zob);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    czb_walk(boards, side, G, rows_all[threadIdx.x >> 6], [&](const CzfGroup &g, const uint32_t (&w)[23], int sd) {
        const CzbKey k = czb_key(w, sd, Z);
        if (!g.live) return;
        const int p = g.g0 + lane;
        int f, n;
        czb_find(bkey, E, k.key, f, n);
        if constexpr (!CHOOSE) {
            first[p] = f, count[p] = n, mirrored[p] = (uint8_t)k.mir;
        } else {
            const uint32_t *row = allowed ? allowed + (size_t)p * CZ_MASK_WORDS : nullptr;
            // an entry's games if it is eligible, else 0 (min_games >= 1 inside the kernel: an entry without games never is);
            // own: its move in the position's OWN orientation
            auto weigh = [&](int i, uint32_t &own) -> uint32_t {
                const uint32_t l = blabel[i], gm = bgames[i];
                if (l >= (uint32_t)CZ_NLABELS || gm < min_games) return 0u;
                own = k.mir == 1 ? (uint32_t)(uint16_t)mirror[l] : l;
                if (own >= (uint32_t)CZ_NLABELS || (row && !((row[own >> 5] >> (own & 31)) & 1u))) return 0u;
                return gm;
            };
            uint32_t pick = 0xFFFFu, own = 0u;
            int at = -1;
            if (mode == 0) {   // the most games, the first of equals
                uint32_t best = 0u;
                for (int i = f; i < f + n; ++i) {
                    const uint32_t gm = weigh(i, own);
                    if (gm > best) best = gm, pick = own, at = i;
                }
            } else {   // in proportion to games: t = rnd * T >> 32 < T, the first entry whose running sum exceeds it
                uint64_t T = 0ull;
                for (int i = f; i < f + n; ++i) T += weigh(i, own);
                const uint64_t t = ((uint64_t)rnd[p] * T) >> 32;
                uint64_t run = 0ull;
                for (int i = f; i < f + n && at < 0; ++i) {
                    const uint32_t gm = weigh(i, own);
                    run += gm;
                    if (gm && run > t) pick = own, at = i;
                }
            }
            played[p] = (uint16_t)pick;
            if (index) index[p] = at;
        }
    });
}

inline dim3 czb_grid(int G, int per_cu) { return dim3(czf_persistent_grid(((G + 63) / 64 + CZB_WAVES - 1) / CZB_WAVES, per_cu)); }
inline bool czb_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

int cz_book_keys(cz_ctx *c, const uint8_t *boards, const uint8_t *side, int G, uint64_t *key, uint8_t *mirrored) {
    CZ_REQUIRE(c && G >= 0, "cz_book_keys: null ctx / negative G");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && key, "cz_book_keys: boards, side, key required");
    CZ_REQUIRE(czb_aligned(key, 8), "cz_book_keys: key must be 8-byte aligned");
    hipLaunchKernelGGL(k_book_keys, czb_grid(G, 2), dim3(64 * CZB_WAVES), 0, c->stream, c->tab, boards, side, G, key, mirrored);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_book_entries(cz_ctx *c, const uint8_t *records, int n, int max_ply, uint64_t *key, uint16_t *label, uint8_t *outcome) {
    CZ_REQUIRE(c && n >= 0, "cz_book_entries: null ctx / negative n");
    CZ_REQUIRE(max_ply >= 0, "cz_book_entries: max_ply >= 0 (0: no bound)");
    if (n == 0) return CZ_OK;
    CZ_REQUIRE(records && key && label && outcome, "cz_book_entries: records, key, label, outcome required");
    CZ_REQUIRE(czb_aligned(records, 16), "cz_book_entries: records must be 16-byte aligned");
    CZ_REQUIRE(czb_aligned(key, 8) && czb_aligned(label, 2), "cz_book_entries: key must be 8-byte, label 2-byte aligned");
    hipLaunchKernelGGL(k_book_entries, czb_grid(n, 4), dim3(64 * CZB_WAVES), 0, c->stream, c->tab, c->tab_mirror, records, n, max_ply, key, label, outcome);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_book_probe(cz_ctx *c, int E, const uint64_t *bkey, const uint8_t *boards, const uint8_t *side, int G, int32_t *first, int32_t *count,
                  uint8_t *mirrored) {
    CZ_REQUIRE(c && G >= 0, "cz_book_probe: null ctx / negative G");
    CZ_REQUIRE(E >= 0, "cz_book_probe: negative E");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && first && count && mirrored, "cz_book_probe: boards, side, first, count, mirrored required");
    CZ_REQUIRE(E == 0 || bkey, "cz_book_probe: bkey required (E > 0)");
    CZ_REQUIRE(czb_aligned(bkey, 8) && czb_aligned(first, 4) && czb_aligned(count, 4), "cz_book_probe: bkey must be 8-byte, first and count 4-byte aligned");
    hipLaunchKernelGGL(k_book_probe<false>, czb_grid(G, 2), dim3(64 * CZB_WAVES), 0, c->stream, c->tab, c->tab_mirror, E, bkey, (const uint16_t *)nullptr,
                       (const uint32_t *)nullptr, boards, side, (const uint32_t *)nullptr, G, 0u, 0, (const uint32_t *)nullptr, first, count, mirrored,
                       (uint16_t *)nullptr, (int32_t *)nullptr);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_book_choose(cz_ctx *c, int E, const uint64_t *bkey, const uint16_t *blabel, const uint32_t *bgames, const uint8_t *boards, const uint8_t *side,
                   const uint32_t *allowed, int G, int min_games, int mode, const uint32_t *rnd, uint16_t *played, int32_t *index) {
    CZ_REQUIRE(c && G >= 0, "cz_book_choose: null ctx / negative G");
    CZ_REQUIRE(E >= 0, "cz_book_choose: negative E");
    CZ_REQUIRE(mode == 0 || mode == 1, "cz_book_choose: mode is 0 (most games) or 1 (sample)");
    CZ_REQUIRE(min_games >= 0, "cz_book_choose: negative min_games");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && played, "cz_book_choose: boards, side, played required");
    CZ_REQUIRE(E == 0 || (bkey && blabel && bgames), "cz_book_choose: bkey, blabel, bgames required (E > 0)");
    CZ_REQUIRE(mode == 0 || rnd, "cz_book_choose: rnd required in mode 1");
    CZ_REQUIRE(czb_aligned(bkey, 8) && czb_aligned(bgames, 4) && czb_aligned(allowed, 4) && czb_aligned(rnd, 4) && czb_aligned(index, 4) &&
                   czb_aligned(blabel, 2) && czb_aligned(played, 2),
               "cz_book_choose: bkey must be 8-byte, bgames, allowed, rnd and index 4-byte, blabel and played 2-byte aligned");
    hipLaunchKernelGGL(k_book_probe<true>, czb_grid(G, 2), dim3(64 * CZB_WAVES), 0, c->stream, c->tab, c->tab_mirror, E, bkey, blabel, bgames, boards, side, allowed, G,
                       (uint32_t)(min_games > 1 ? min_games : 1), mode, rnd, (int32_t *)nullptr, (int32_t *)nullptr, (uint8_t *)nullptr, played, index);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
