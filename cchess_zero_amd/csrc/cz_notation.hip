// cz_notation.hip — cz_games_read: cz_games_replay for games whose moves are TOKENS, a move label or a move named in WXF /
// Chinese notation (cz_notation.h: "C2=5" as four bytes), both kinds in one launch.  A named move can only be read against the
// position it is played in, and the replay is the one place that has every game's position at every ply: the lane keeps its
// game's board across all plies and the ply's legal list lies in its LDS row.  So the body is k_games_replay's
// (czg_replay_body, cz_games_body.h) with the move found by czn_pick: the token's kind as a set of squares, built once per ply
// from the board in the lane's LDS row, then at most 128 listed moves tried against the token, four per trip of a wave-wide
// loop, their labels read from the row; matches counted, one match made.  No scratch at either rule level.
// srcdst (label -> squares, 4 172 bytes) is read once per listed move: it is STAGED in LDS, 2 088 halfwords beside the body's
// 48.0 KB — 52.0 KB per wave, under a third of a CU's 160 KB, so the launch shape of cz_games_replay (persistent grid, three
// waves per CU) carries over.
#include "cz_games_body.h"

static_assert(CZG_AMBIGUOUS == CZ_GAME_AMBIGUOUS, "cz_games.h restates include/cchess_hip.h");

namespace {

constexpr int CZN_SRCDST = (CZ_NLABELS + 7) / 8 * 8;   // halfwords of the staged table: whole 16-byte pieces

template <int RULES>
__global__ __launch_bounds__(64) void k_games_read(const CzmTables *__restrict__ gtab, const uint16_t *__restrict__ srcdst,
                                                   const uint8_t *__restrict__ start_boards, const uint8_t *__restrict__ start_side,
                                                   const uint32_t *__restrict__ tokens, int stride, const int32_t *__restrict__ len,
                                                   const int8_t *__restrict__ result, int G, const int32_t *__restrict__ rec_offset, int total,
                                                   uint8_t *__restrict__ records, int32_t *__restrict__ valid, uint8_t *__restrict__ status,
                                                   uint8_t *__restrict__ end_flags, uint8_t *__restrict__ final_boards, uint8_t *__restrict__ final_side,
                                                   uint16_t *__restrict__ labels_out) {
    __shared__ __attribute__((aligned(16))) uint16_t sdl[CZN_SRCDST];
    for (int i = threadIdx.x; i < CZN_SRCDST; i += 64) sdl[i] = i < CZ_NLABELS ? srcdst[i] : (uint16_t)0;   // the body's first fence covers it
    czg_replay_body<RULES, uint32_t>(gtab, srcdst, sdl, start_boards, start_side, tokens, stride, len, result, G, rec_offset, total, records, valid,
                                     status, end_flags, final_boards, final_side, labels_out);
}

}  // namespace

int cz_games_read(cz_ctx *c, const uint8_t *start_boards, const uint8_t *start_side, const uint32_t *tokens, int stride, const int32_t *len,
                  const int8_t *result, int G, int rules, const int32_t *rec_offset, int total, uint8_t *records, int32_t *valid, uint8_t *status,
                  uint8_t *end_flags, uint8_t *final_boards, uint8_t *final_side, uint16_t *labels_out) {
    CZ_REQUIRE(c && G >= 0, "cz_games_read: null ctx / negative G");
    CZ_REQUIRE(stride >= 0 && stride <= 65535 && total >= 0, "cz_games_read: 0 <= stride <= 65535 and total >= 0 required");
    CZ_REQUIRE(rules == 0 || rules == 1, "cz_games_read: rules is 0 (capture) or 1 (king-safe)");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(tokens && len && result && rec_offset && valid && status && end_flags,
               "cz_games_read: tokens, len, result, rec_offset, valid, status, end_flags required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15u) == 0, "cz_games_read: records must be 16-byte aligned");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(tokens) & 3u) == 0 && (reinterpret_cast<uintptr_t>(labels_out) & 1u) == 0,
               "cz_games_read: tokens must be 4-byte and labels_out 2-byte aligned");
    CZ_REQUIRE(!final_boards || final_side, "cz_games_read: final_boards needs final_side");
    const dim3 grid(czf_persistent_grid((G + 63) / 64, 3));   // 52.0 KB of LDS per wave: three waves per CU
#define CZN_LAUNCH(R) hipLaunchKernelGGL((k_games_read<R>), grid, dim3(64), 0, c->stream, c->mask_tab, c->tab.srcdst, start_boards, start_side, tokens, stride, \
                                         len, result, G, rec_offset, total, records, valid, status, end_flags, final_boards, final_side, labels_out)
    if (rules) CZN_LAUNCH(1);
    else CZN_LAUNCH(0);
#undef CZN_LAUNCH
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
