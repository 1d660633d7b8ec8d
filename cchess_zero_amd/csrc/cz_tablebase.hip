// cz_tablebase.hip — cz_tb_pass, cz_tb_probe, cz_tb_boards: endgame tablebases by retrograde analysis (include/cchess_hip.h:
// TABLEBASES; cz_tablebase.h: the index mapping and one index's step).  Three kernels in the frame of cz_posframe.h: one lane per
// index or position, one wave per group of 64, workgroups of one wave, persistent.
// k_tb_pass is one pass over a whole table IN PLACE.  A lane's board is MADE from its index in registers — there is no board
// traffic at all —, czk_position<LIST> lists its king-safe moves into the lane's LDS row, and every move's child is an index
// computed from the parent's digits: 2 bytes gathered per child, from this table or from the table of the signature without
// the piece taken (their pointers and the radices travel in the kernel-argument struct).  A lane whose entry is decided runs
// along on an empty board (cztb_step's go = false), a group without an undecided lane is skipped after its one 128-byte load —
// in late passes that is most groups.  Values written in pass d have plies == d and count as not settled for every reader of
// the launch, so which of a neighbour's stores a wave sees decides nothing: no fence, no flag, no second buffer.  The LDS is
// k_movegen_kingsafe's list form less the staged boards' surplus: 64 list rows, czk_position's 34 scratch words per lane and
// the tables, 26.3 KB per wave, six waves per CU.
#include "cz_internal.h"
#include "cz_posframe.h"
#include "cz_tablebase.h"

static_assert(CZTB_ILLEGAL == CZ_TB_ILLEGAL && CZTB_UNKNOWN == CZ_TB_UNKNOWN && CZTB_MISS == CZ_TB_MISS && CZTB_MAX_SLOTS == CZ_TB_MAX_SLOTS,
              "cz_tablebase.h restates include/cchess_hip.h");

namespace {

struct CztbPassArgs {
    CztbDesc d;
    int16_t *table;                         // [d.entries], read and written by every wave of the launch
    const int16_t *sub[CZTB_MAX_SLOTS];     // the finished table without slot j, NULL for a king
    int pass;
    unsigned long long *decided;
};

__global__ __launch_bounds__(64) void k_tb_pass(const CzmTables *__restrict__ gtab, const uint16_t *__restrict__ srcdst, const CztbPassArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[64 * CZF_LROW];       // the 64 list rows
    __shared__ uint32_t slots[CZK_SCRATCH * 64];                                  // [word][lane]
    __shared__ __attribute__((aligned(16))) CzmTables T;
    const int lane = threadIdx.x;
    if (lane < (int)(sizeof(CzmTables) / 16)) reinterpret_cast<uint4 *>(&T)[lane] = reinterpret_cast<const uint4 *>(gtab)[lane];
    const uint32_t entries = a.d.entries, ngroups = (entries + 63u) >> 6;
    const uint16_t *const lrow = reinterpret_cast<const uint16_t *>(rows + lane * CZF_LROW);
    uint16_t *const lput = reinterpret_cast<uint16_t *>(rows + lane * CZF_LROW);
    uint32_t mine = 0u;   // indices this lane decided
    for (uint32_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        const uint32_t i = grp * 64u + (uint32_t)lane;
        const bool live = i < entries;
        int cur = CZTB_UNKNOWN;
        if (a.pass && live) cur = a.table[i];   // the group's one 128-byte load
        const bool go = live && cur == CZTB_UNKNOWN;
        if (!CZM_ANY(go)) continue;   // wave-uniform
        CZF_WAVE_FENCE();   // the previous group's list has been read (and the tables are in place)
        const int v = cztb_step(a.d, i, cur, a.pass, go, T, srcdst,
            [&](int k) -> uint32_t & { return slots[k * 64 + lane]; },
            [lput](int k, int label) { lput[k & 127] = (uint16_t)label; },   // k < 128: the slots hold at most 121 moves
            []() {},
            []() { CZF_WAVE_FENCE(); },   // the list is complete
            [lrow](int k) { return lrow[k & 127]; },
            [&a](int t, uint32_t at) -> int {
                const int16_t *p = a.table;
#pragma unroll
                for (int k = 0; k < CZTB_MAX_SLOTS; ++k) p = t == k ? a.sub[k] : p;
                return p ? (int)p[at] : CZTB_UNKNOWN;
            });
        if (go && (a.pass == 0 || v != CZTB_UNKNOWN)) a.table[i] = (int16_t)v;
        mine += (go && a.pass != 0 && v != CZTB_UNKNOWN) ? 1u : 0u;
    }
    // one wave-reduced add per wave
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) mine += __shfl_xor(mine, s, 64);
    if (lane == 0 && mine && a.decided) atomicAdd(a.decided, (unsigned long long)mine);
}

__global__ __launch_bounds__(64) void k_tb_probe(const CztbDesc d, const int16_t *__restrict__ table, const uint8_t *__restrict__ boards,
                                                 const uint8_t *__restrict__ side, int G, int16_t *__restrict__ value, int32_t *__restrict__ index) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[CZF_BOARD_WORDS + 4];   // the boards and the word lane 63's funnel shift reads behind them
    const int lane = threadIdx.x;
    CzfLoader ld(boards, side, G, lane);
    ld.request(blockIdx.x);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        CZF_WAVE_FENCE();   // the previous group's boards are in registers
        const int sd = ld.stage(rows, g);
        CZF_WAVE_FENCE();
        uint32_t w[23];
        czf_unpack(rows, lane, g.live, w);
        ld.request(grp + gridDim.x);
        uint32_t at = 0u;
        const int st = cztb_rank(d, w, sd, &at);   // a dead lane's empty board is a miss
        int v = st;
        if (st == 0 && at < d.entries) v = table[at];
        if (g.live) {
            value[g.g0 + lane] = (int16_t)v;
            if (index) index[g.g0 + lane] = st == 0 ? (int32_t)at : -1;
        }
    }
}

__global__ __launch_bounds__(64) void k_tb_boards(const CztbDesc d, const int32_t *__restrict__ index, int G, uint8_t *__restrict__ boards,
                                                  uint8_t *__restrict__ side) {
    __shared__ __attribute__((aligned(16))) uint32_t rows[CZF_BOARD_WORDS];   // the group's 64 boards as they leave: 5 760 bytes
    const int lane = threadIdx.x;
    uint16_t *const rows16 = reinterpret_cast<uint16_t *>(rows);
    for (int grp = blockIdx.x; grp < czf_ngroups(G); grp += gridDim.x) {
        const CzfGroup g = czf_group(grp, G, lane);
        const int32_t ix = g.live ? index[g.g0 + lane] : -1;
        const bool in = ix >= 0 && (uint32_t)ix < d.entries;
        int sq[CZTB_MAX_SLOTS], dg[CZTB_MAX_SLOTS];
        bool overlap;
        const int sd = cztb_unrank(d, in ? (uint32_t)ix : 0u, sq, dg, &overlap);
        uint32_t w[23];
        cztb_words(d, sq, in && !overlap, w);
        CZF_WAVE_FENCE();   // the previous group's rows have left
#pragma unroll
        for (int k = 0; k < 22; ++k) {   // the lane's 90 bytes start at byte 90 * lane: halfword 45 * lane
            rows16[45 * lane + 2 * k] = (uint16_t)w[k];
            rows16[45 * lane + 2 * k + 1] = (uint16_t)(w[k] >> 16);
        }
        rows16[45 * lane + 44] = (uint16_t)w[22];
        if (g.live && side) side[g.g0 + lane] = (uint8_t)(in ? sd : 0);
        CZF_WAVE_FENCE();
        uint8_t *const dst = boards + (size_t)g.g0 * CZ_NSQ;   // 16-byte aligned: g0 * 90 is a multiple of 5 760
        const int nbytes = g.np * CZ_NSQ;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int p = lane + 64 * k;
            if (16 * p + 16 <= nbytes) reinterpret_cast<uint4 *>(dst)[p] = reinterpret_cast<const uint4 *>(rows)[p];
        }
        const int full = nbytes & ~15;   // a batch's last group: its ragged piece byte by byte, never past the batch
        if (lane < nbytes - full) dst[full + lane] = reinterpret_cast<const uint8_t *>(rows)[full + lane];
    }
}

}  // namespace

// the signature -> its descriptor, or CZ_EINVAL with `who` in the text (cz_internal.h: cz_tablebase_set.hip reads signatures too)
int tb_desc(const char *who, const char *signature, CztbDesc *d) {
    const int rc = cztb_parse(signature, d);
    if (rc == 0) return CZ_OK;
    static const char *const why[] = {"", "red pieces, '-', black pieces, of the letters KRNCPAB", "each side starts with its one K",
                                      "letters in the order KRNCPAB, at most two of R N C A B and five P", "more than 10 slots or 2^31 - 1 entries"};
    cz_set_error("%s: bad signature \"%s\": %s", who, signature ? signature : "(null)", why[-rc]);
    return CZ_EINVAL;
}

int cz_tb_entries(const char *signature, long long *entries, int *n_slots) {
    CztbDesc d;
    if (const int rc = tb_desc("cz_tb_entries", signature, &d)) return rc;
    if (entries) *entries = (long long)d.entries;
    if (n_slots) *n_slots = d.n;
    return CZ_OK;
}

int cz_tb_pass(cz_ctx *c, const char *signature, int16_t *table, const int16_t *const *sub, int pass, unsigned long long *decided) {
    CZ_REQUIRE(c, "cz_tb_pass: null ctx");
    CztbPassArgs a;
    if (const int rc = tb_desc("cz_tb_pass", signature, &a.d)) return rc;
    CZ_REQUIRE(pass >= 0 && pass <= 32000, "cz_tb_pass: pass is 0 .. 32000 (a value is an int16)");
    CZ_REQUIRE(table && (reinterpret_cast<uintptr_t>(table) & 1u) == 0, "cz_tb_pass: table required, 2-byte aligned");
    CZ_REQUIRE(pass == 0 || (sub && decided), "cz_tb_pass: sub and decided required from pass 1 on");
    CZ_REQUIRE(!decided || (reinterpret_cast<uintptr_t>(decided) & 7u) == 0, "cz_tb_pass: decided must be 8-byte aligned");
    for (int k = 0; k < CZTB_MAX_SLOTS; ++k) {
        const bool king = k < a.d.n && (a.d.code[k] == 1 || a.d.code[k] == 8);
        a.sub[k] = (pass && k < a.d.n && !king) ? sub[k] : nullptr;
        if (pass && k < a.d.n && !king && (!a.sub[k] || (reinterpret_cast<uintptr_t>(a.sub[k]) & 1u))) {
            cz_set_error("cz_tb_pass: sub[%d] (the table of \"%s\" without slot %d) required, 2-byte aligned", k, signature, k);
            return CZ_EINVAL;
        }
    }
    a.table = table, a.pass = pass, a.decided = decided;
    const int ngroups = (int)((a.d.entries + 63u) >> 6);
    hipLaunchKernelGGL(k_tb_pass, dim3(czf_persistent_grid(ngroups, 6)), dim3(64), 0, c->stream, c->mask_tab, c->tab.srcdst, a);   // 26.3 KB of LDS per wave
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_tb_probe(cz_ctx *c, const char *signature, const int16_t *table, const uint8_t *boards, const uint8_t *side, int G, int16_t *value,
                int32_t *index) {
    CZ_REQUIRE(c && G >= 0, "cz_tb_probe: null ctx / negative G");
    CztbDesc d;
    if (const int rc = tb_desc("cz_tb_probe", signature, &d)) return rc;
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(table && boards && side && value, "cz_tb_probe: table, boards, side, value required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(table) & 1u) == 0 && (reinterpret_cast<uintptr_t>(value) & 1u) == 0 && (reinterpret_cast<uintptr_t>(index) & 3u) == 0,
               "cz_tb_probe: table and value must be 2-byte, index 4-byte aligned");
    hipLaunchKernelGGL(k_tb_probe, dim3(czf_persistent_grid((G + 63) / 64, 16)), dim3(64), 0, c->stream, d, table, boards, side, G, value, index);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_tb_boards(cz_ctx *c, const char *signature, const int32_t *index, int G, uint8_t *boards, uint8_t *side) {
    CZ_REQUIRE(c && G >= 0, "cz_tb_boards: null ctx / negative G");
    CztbDesc d;
    if (const int rc = tb_desc("cz_tb_boards", signature, &d)) return rc;
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(index && boards, "cz_tb_boards: index, boards required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(index) & 3u) == 0, "cz_tb_boards: index must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(boards) & 15u) { cz_set_error("cz_tb_boards: boards must be 16-byte aligned"); return CZ_EINVAL; }
    hipLaunchKernelGGL(k_tb_boards, dim3(czf_persistent_grid((G + 63) / 64, 16)), dim3(64), 0, c->stream, d, index, G, boards, side);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
