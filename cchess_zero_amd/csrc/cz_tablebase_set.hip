// cz_tablebase_set.hip — cz_tb_set_create / _destroy / _probe: several finished tables behind one handle, and k_tb_probe_set, the
// ONE launch that answers a batch of positions of any material against all of them (include/cchess_hip.h: TABLE SETS).
// Tablebase.probe groups a mixed batch on the host and launches one k_tb_probe per signature present; the self-play and match
// loops cannot wait for the host every ply, so their adjudication (cz_selfplay.hip, cz_match.hip) probes through this kernel.
// The kernel is in the frame of cz_posframe.h like k_tb_probe: one lane per position, one wave per group of 64, workgroups of one
// wave, persistent.  A lane takes its board's four bit planes once (cztb_planes), a board of more than CZTB_MAX_SLOTS pieces is a
// miss there and then — in self-play that is almost every root, and a group without any other lane skips everything below —,
// the others compute their material key (cztb_material_key) and find it among the set's sorted keys by a binary search of eight
// steps in LDS.  The lanes of a wave hold DIFFERENT entries in general, and cztb_rank / cztb_digit want a wave-uniform
// descriptor (their selects on code, dom, ord and radix are scalar then): a WATERFALL loop takes the first pending lane's entry,
// reads its number into a scalar register, loads that one 72-byte directory entry with scalar loads, and the lanes that hold it rank their position
// and read their 2 bytes; a wave of one signature runs the loop once, a wave of misses never.
// LDS: the staged boards (cz_posframe.h) and the keys, 7 824 bytes per wave; no scratch, no register array indexed at run time,
// no __syncthreads.
#include <vector>

#include "cz_internal.h"
#include "cz_posframe.h"
#include "cz_tablebase.h"

static_assert(CZ_TB_SET_MAX == CZTB_SET_MAX, "cz_tablebase.h restates include/cchess_hip.h");

// one entry of a set's directory, in device memory; the entries are in ascending key order
struct CztbSetEntry {
    CztbDesc d;
    int32_t which;           // the signature's place in the order given to cz_tb_set_create
    const int16_t *table;    // [d.entries], the caller's
};
static_assert(sizeof(CztbSetEntry) == 72, "a directory entry is 18 dwords: one scalar load sequence");

struct cz_tb_set {
    int device;
    int n;
    int held;                   // consumers that have it attached (cz_tb_set_hold)
    void *block;                // the one allocation behind keys and dir
    const uint64_t *keys;       // [n] ascending
    const CztbSetEntry *dir;    // [n]
};

namespace {

// ROWS false: the boards are 90 bytes apart, staged through LDS by CzfLoader; true: rows of board_stride bytes (a multiple of 16,
// 16-byte aligned), every lane loads its own
template <bool ROWS>
__global__ __launch_bounds__(64) void k_tb_probe_set(const uint64_t *__restrict__ keys, const CztbSetEntry *__restrict__ dir, int n,
                                                     const uint8_t *__restrict__ boards, int board_stride, const uint8_t *__restrict__ side,
                                                     int side_stride, const uint16_t *__restrict__ moved, int G, int16_t *__restrict__ value,
                                                     int32_t *__restrict__ which) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[ROWS ? 4 : CZF_BOARD_WORDS + 4];   // the boards and the word lane 63's funnel shift reads behind them
    __shared__ uint64_t skeys[CZ_TB_SET_MAX];                                                  // the sorted keys, ~0 behind the last
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < CZ_TB_SET_MAX / 64; ++k) skeys[lane + 64 * k] = lane + 64 * k < n ? keys[lane + 64 * k] : ~0ull;
    CzfLoader ld(boards, side, G, lane);
    if constexpr (!ROWS) ld.request(blockIdx.x);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        uint32_t w[23];
        int sd = 0;
        if constexpr (ROWS) {
            uint4 v[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = make_uint4(0, 0, 0, 0);
            if (g.live) {
                const uint4 *src = reinterpret_cast<const uint4 *>(boards + (size_t)(g.g0 + lane) * board_stride);
#pragma unroll
                for (int k = 0; k < 6; ++k) v[k] = src[k];
                sd = side[(size_t)(g.g0 + lane) * side_stride] ? 1 : 0;
            }
#pragma unroll
            for (int k = 0; k < 23; ++k) w[k] = (k & 3) == 0 ? v[k >> 2].x : (k & 3) == 1 ? v[k >> 2].y : (k & 3) == 2 ? v[k >> 2].z : v[k >> 2].w;
            w[22] &= 0x0000FFFFu;
            CZF_WAVE_FENCE();   // the keys are in place
        } else {
            CZF_WAVE_FENCE();   // the previous group's boards are in registers (and the keys are in place)
            sd = ld.stage(rows, g);
            CZF_WAVE_FENCE();
            czf_unpack(rows, lane, g.live, w);
            ld.request(grp + gridDim.x);
        }
        const bool asked = g.live && (!moved || moved[g.g0 + lane] < CZ_NLABELS);
        const CztbPlanes P = cztb_planes(w);
        // the cheap path: more pieces than any table has slots (or a byte above 15, or a lane nobody asks for) is a miss
        const bool few = asked && P.high == 0u && czm_popcnt(cztb_occupied(P)) <= CZTB_MAX_SLOTS;
        int v = CZTB_MISS, wh = -1;
        if (CZM_ANY(few)) {   // wave-uniform
            const uint64_t key = few ? cztb_material_key(P) : ~0ull;   // ~0 is no key: it has bit 63
            const int lo = cztb_set_find(skeys, n, key);   // the lane's entry, -1: a miss
            bool pending = few && lo >= 0;
            // The waterfall.  The loop's control flow is wave-uniform and the entry is loaded BEFORE any lane compares its own
            // number with it: inside a branch on `lo == e` the compiler addresses the entry by the lane's lo and the descriptor
            // becomes sixty vector loads per lane.
            for (unsigned long long m = __ballot(pending); m != 0ull; m = __ballot(pending)) {
                const int e = __builtin_amdgcn_readlane(lo, __ffsll(m) - 1);   // the first pending lane's entry, in a scalar register
                CztbSetEntry E;   // as 18 dwords: loaded field by field, the descriptor's byte arrays would come through vector loads
                {
                    const uint32_t *src = reinterpret_cast<const uint32_t *>(dir + e);
                    uint32_t raw[sizeof(CztbSetEntry) / 4];
#pragma unroll
                    for (int k = 0; k < (int)(sizeof(CztbSetEntry) / 4); ++k) raw[k] = src[k];
                    __builtin_memcpy(&E, raw, sizeof(E));
                }
                const bool mine = pending && lo == e;
                uint32_t at = 0u;
                const int st = cztb_rank(E.d, P, sd, &at);   // every lane runs along; the key says it is no CZTB_MISS for `mine`
                if (mine) {
                    v = st;
                    if (st == 0 && at < E.d.entries) v = E.table[at];
                    wh = E.which;
                }
                pending = pending && !mine;
            }
        }
        if (g.live) {
            value[g.g0 + lane] = (int16_t)v;
            if (which) which[g.g0 + lane] = wh;
        }
    }
}

}  // namespace

int cz_tb_set_create(cz_ctx *c, int n, const char *const *signatures, const int16_t *const *tables, cz_tb_set **out) {
    CZ_REQUIRE(out, "cz_tb_set_create: null out");
    *out = nullptr;
    CZ_REQUIRE(c && signatures && tables, "cz_tb_set_create: null ctx / signatures / tables");
    if (n < 1 || n > CZ_TB_SET_MAX) {
        cz_set_error("cz_tb_set_create: 1 <= n <= %d signatures (the kernel keeps the keys in LDS)", CZ_TB_SET_MAX);
        return CZ_EINVAL;
    }
    std::vector<CztbSetEntry> dir((size_t)n);
    std::vector<uint64_t> keys((size_t)n);
    std::vector<int> order((size_t)n);
    for (int i = 0; i < n; ++i) {
        CztbSetEntry &e = dir[i];
        if (const int rc = tb_desc("cz_tb_set_create", signatures[i], &e.d)) return rc;
        if (!tables[i] || (reinterpret_cast<uintptr_t>(tables[i]) & 1u)) {
            cz_set_error("cz_tb_set_create: tables[%d] (the table of \"%s\") required, 2-byte aligned", i, signatures[i]);
            return CZ_EINVAL;
        }
        e.which = i, e.table = tables[i];
        keys[i] = cztb_desc_key(e.d);
    }
    if (const int twice = cztb_set_sort(n, keys.data(), order.data())) {
        cz_set_error("cz_tb_set_create: signature \"%s\" given twice", signatures[order[twice - 1]]);
        return CZ_EINVAL;
    }
    std::vector<CztbSetEntry> sdir((size_t)n);
    std::vector<uint64_t> skeys((size_t)n);
    for (int i = 0; i < n; ++i) sdir[i] = dir[order[i]], skeys[i] = keys[order[i]];
    cz_tb_set *s = new cz_tb_set();
    s->device = c->device, s->n = n, s->held = 0, s->block = nullptr;
    uint64_t *dkeys = nullptr;
    CztbSetEntry *ddir = nullptr;
    int rc = carve_alloc(&s->block, c->stream, false, "cz_tb_set_create", [&](Carver &k) {
        dkeys = k.take<uint64_t>((size_t)n);
        ddir = k.take<CztbSetEntry>((size_t)n);
    });
    if (rc == CZ_OK) {
        // pageable host memory: both copies have left the vectors when the calls return
        hipError_t e = hipMemcpyAsync(dkeys, skeys.data(), sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ddir, sdir.data(), sizeof(CztbSetEntry) * (size_t)n, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            cz_set_error("cz_tb_set_create: the directory's upload failed: %s", hipGetErrorString(e));
            rc = CZ_EHIP;
        }
    }
    if (rc != CZ_OK) {
        if (s->block) (void)hipFree(s->block);
        delete s;
        return rc;
    }
    s->keys = dkeys, s->dir = ddir;
    *out = s;
    return CZ_OK;
}

int cz_tb_set_destroy(cz_tb_set *s) {
    if (!s) return CZ_OK;
    CZ_REQUIRE(s->held == 0, "cz_tb_set_destroy: the set is attached: cz_selfplay_set_tablebase(ctx, NULL) / cz_match_set_tablebase(match, NULL) first");
    (void)hipDeviceSynchronize();   // a probe of any stream may still read the directory
    (void)hipFree(s->block);
    delete s;
    return CZ_OK;
}

void cz_tb_set_hold(cz_tb_set *s, int delta) {
    if (s) s->held += delta;
}

int cz_tb_set_attachable(const char *api, const char *handle, const cz_ctx *c, const cz_tb_set *set, int rules) {
    if (!set) return CZ_OK;
    if (rules != 1) {
        cz_set_error("%s_set_tablebase: %s_set_rules(%s, 1) first (a table holds values under xiangqi rules)", api, api, handle);
        return CZ_EINVAL;
    }
    if (set->device != c->device) {
        cz_set_error("%s_set_tablebase: the set was made on device %d, the %s runs on device %d", api, set->device, handle, c->device);
        return CZ_EINVAL;
    }
    return CZ_OK;
}

int cz_tb_set_probe_strided(cz_ctx *c, const cz_tb_set *s, const uint8_t *boards, int board_stride, const uint8_t *side, int side_stride,
                            const uint16_t *moved, int G, int16_t *value, int32_t *which) {
    const int grid = czf_persistent_grid((G + 63) / 64, 16);
    if (board_stride == CZ_NSQ && side_stride == 1) {
        hipLaunchKernelGGL(k_tb_probe_set<false>, dim3(grid), dim3(64), 0, c->stream, s->keys, s->dir, s->n, boards, board_stride, side, side_stride, moved, G,
                           value, which);
    } else {
        CZ_REQUIRE(board_stride >= 96 && (board_stride & 15) == 0 && (reinterpret_cast<uintptr_t>(boards) & 15u) == 0 && side_stride >= 1,
                   "cz_tb_set_probe: rows of boards are a multiple of 16 bytes, at least 96, 16-byte aligned");
        hipLaunchKernelGGL(k_tb_probe_set<true>, dim3(grid), dim3(64), 0, c->stream, s->keys, s->dir, s->n, boards, board_stride, side, side_stride, moved, G,
                           value, which);
    }
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_tb_set_probe(cz_ctx *c, const cz_tb_set *s, const uint8_t *boards, const uint8_t *side, int G, int16_t *value, int32_t *which) {
    CZ_REQUIRE(c && G >= 0, "cz_tb_set_probe: null ctx / negative G");
    CZ_REQUIRE(s, "cz_tb_set_probe: null set");
    CZ_REQUIRE(s->device == c->device, "cz_tb_set_probe: the set was made on another device");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && value, "cz_tb_set_probe: boards, side, value required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(value) & 1u) == 0 && (reinterpret_cast<uintptr_t>(which) & 3u) == 0,
               "cz_tb_set_probe: value must be 2-byte, which 4-byte aligned");
    return cz_tb_set_probe_strided(c, s, boards, CZ_NSQ, side, 1, nullptr, G, value, which);
}
