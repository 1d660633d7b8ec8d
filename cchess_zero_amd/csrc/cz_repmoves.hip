// cz_repmoves.hip — cz_repetition_moves: the two-ply repetition verdicts of cz_repmoves.h on G positions and the game records
// the caller keeps (as cz_repetition_chase takes them).  One wave64 per game, CZV_WAVES waves to a workgroup that share the
// tables; a wave walks its games with a stride.  One launch, no atomics, no child board in memory.
#include "cz_internal.h"
#include "cz_repmoves.h"

namespace {

constexpr int CZV_WAVES = 2;   // 16 KB of tables + 31.9 KB per wave: 80 KB of LDS per workgroup, two workgroups per CU

template <bool CHASE>
__global__ __launch_bounds__(64 * CZV_WAVES) void k_repetition_moves(CzTables tab, const CzmTables *__restrict__ gtab,
                                                                     const uint8_t *__restrict__ boards, const uint8_t *__restrict__ side,
                                                                     const uint64_t *__restrict__ keys, const uint8_t *__restrict__ in_check,
                                                                     const uint64_t *__restrict__ chase, int stride,
                                                                     const int32_t *__restrict__ len, const int32_t *__restrict__ window, int G,
                                                                     int fold, uint16_t *__restrict__ moves, uint16_t *__restrict__ count,
                                                                     uint8_t *__restrict__ verdict, uint16_t *__restrict__ reply,
                                                                     uint8_t *__restrict__ reply_verdict, uint32_t *__restrict__ allowed,
                                                                     uint8_t *__restrict__ summary) {
    __shared__ CzvShared S;
    __shared__ CzvWave Wv[CZV_WAVES];
    czv_load_shared(S, gtab, tab.srcdst, tab.zob, threadIdx.x, 64 * CZV_WAVES);
    __syncthreads();   // the only workgroup-wide one: from here on every wave walks its own games
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int g = blockIdx.x * CZV_WAVES + wv; g < G; g += gridDim.x * CZV_WAVES) {
        const int L = __builtin_amdgcn_readfirstlane(len[g]);
        CzvHistory H;
        H.valid = L >= 1 && L <= stride;   // a length outside the record: no verdicts, nothing behind the row is read
        H.keys = keys + (size_t)g * stride;
        H.chk = in_check + (size_t)g * stride;
        H.chase = CHASE ? chase + (size_t)g * stride * 4 : nullptr;
        H.imask = 0x7fffffff;
        H.wcap = 0x7fffffff;
        H.n0 = H.valid ? L - 1 : 0;
        H.w0 = H.valid ? (window ? max(0, min(__builtin_amdgcn_readfirstlane(window[g]), H.n0)) : H.n0) : 0;
        H.key0 = H.valid ? H.keys[H.n0] : 0ull;
        H.chk0 = H.valid && H.chk[H.n0] != 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) H.rec0[k] = (CHASE && H.valid) ? H.chase[(size_t)H.n0 * 4 + k] : 0ull;
        CzvOut out;
        out.moves = moves ? moves + (size_t)g * CZD_MAXMOVES : nullptr;
        out.count = count ? count + g : nullptr;
        out.verdict = verdict ? verdict + (size_t)g * CZD_MAXMOVES : nullptr;
        out.reply = reply ? reply + (size_t)g * CZD_MAXMOVES : nullptr;
        out.reply_verdict = reply_verdict ? reply_verdict + (size_t)g * CZD_MAXMOVES : nullptr;
        out.allowed = allowed ? allowed + (size_t)g * CZ_MASK_WORDS : nullptr;
        out.summary = summary ? summary + g : nullptr;
        wave_repetition_moves<CHASE>(Wv[wv], S, boards + (size_t)g * CZ_NSQ, side[g] ? 1 : 0, H, fold, lane, out);
    }
}

// The avoid step of a match or of self-play: slot g's root position (rr.board, gathered at rr.slot_ply[g]) against the slot's
// rings.  The ring entry of the current ply is written later, in choose: the current position's key, flag and record are
// rr.root_*; the window is wave_root_history's, min(root_rr, ply, 63), and no window grows past 63.
template <bool CHASE>
__global__ __launch_bounds__(64 * CZV_WAVES) void k_root_avoid(CzTables tab, const CzmTables *__restrict__ gtab, CzRootRules rr, int G) {
    __shared__ CzvShared S;
    __shared__ CzvWave Wv[CZV_WAVES];
    czv_load_shared(S, gtab, tab.srcdst, tab.zob, threadIdx.x, 64 * CZV_WAVES);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int g = blockIdx.x * CZV_WAVES + wv; g < G; g += gridDim.x * CZV_WAVES) {
        const int ply = __builtin_amdgcn_readfirstlane(rr.slot_ply[g]);
        if (ply < 0) {   // a parked slot
            if (lane == 0) rr.avoid_sum[g] = 0;
            continue;
        }
        CzvHistory H;
        H.valid = true;
        H.keys = rr.ring_key + (size_t)g * 64;
        H.chk = rr.ring_check + (size_t)g * 64;
        H.chase = CHASE ? rr.ring_chase + (size_t)g * 64 * 4 : nullptr;
        H.imask = 63;
        H.wcap = 63;
        H.n0 = ply;
        H.w0 = max(0, min(min(__builtin_amdgcn_readfirstlane(rr.slot_rr[g]), ply), 63));
        H.key0 = rr.root_key[g];
        H.chk0 = (rr.flags[g] & CZ_POS_IN_CHECK) != 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) H.rec0[k] = CHASE ? rr.root_chase[(size_t)g * 4 + k] : 0ull;
        CzvOut out = {nullptr, nullptr, nullptr, nullptr, nullptr, rr.safe + (size_t)g * CZ_MASK_WORDS, rr.avoid_sum + g};
        wave_repetition_moves<CHASE>(Wv[wv], S, rr.board + (size_t)g * CZ_NSQ, rr.side[g] ? 1 : 0, H, rr.fold, lane, out);
    }
}

}  // namespace

int czv_root_avoid(cz_ctx *c, const CzRootRules &rr, int G, int chase) {
    if (G <= 0) return CZ_OK;
    const dim3 grid(czf_persistent_grid((G + CZV_WAVES - 1) / CZV_WAVES, 2)), block(64 * CZV_WAVES);
    if (chase) hipLaunchKernelGGL(k_root_avoid<true>, grid, block, 0, c->stream, c->tab, c->mask_tab, rr, G);
    else hipLaunchKernelGGL(k_root_avoid<false>, grid, block, 0, c->stream, c->tab, c->mask_tab, rr, G);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}

int cz_repetition_moves(cz_ctx *c, const uint8_t *boards, const uint8_t *side, const uint64_t *keys, const uint8_t *in_check,
                        const uint64_t *chase, int stride, const int32_t *len, const int32_t *window, int G, int fold, uint16_t *moves,
                        uint16_t *count, uint8_t *verdict, uint16_t *reply, uint8_t *reply_verdict, uint32_t *allowed, uint8_t *summary) {
    CZ_REQUIRE(c && G >= 0, "cz_repetition_moves: null ctx / negative G");
    CZ_REQUIRE(fold >= 2 && fold <= 8, "cz_repetition_moves: 2 <= fold <= 8");
    CZ_REQUIRE(stride >= 1, "cz_repetition_moves: stride >= 1");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(boards && side && keys && in_check && len, "cz_repetition_moves: boards, side, keys, in_check, len required");
    CZ_REQUIRE(moves || count || verdict || reply || reply_verdict || allowed || summary, "cz_repetition_moves: no output requested");
    if (moves && (reinterpret_cast<uintptr_t>(moves) & 15u)) { cz_set_error("cz_repetition_moves: moves must be 16-byte aligned"); return CZ_EINVAL; }
    const dim3 grid(czf_persistent_grid((G + CZV_WAVES - 1) / CZV_WAVES, 2)), block(64 * CZV_WAVES);
    if (chase)
        hipLaunchKernelGGL(k_repetition_moves<true>, grid, block, 0, c->stream, c->tab, c->mask_tab, boards, side, keys, in_check, chase, stride, len,
                           window, G, fold, moves, count, verdict, reply, reply_verdict, allowed, summary);
    else
        hipLaunchKernelGGL(k_repetition_moves<false>, grid, block, 0, c->stream, c->tab, c->mask_tab, boards, side, keys, in_check, chase, stride, len,
                           window, G, fold, moves, count, verdict, reply, reply_verdict, allowed, summary);
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
