// cz_games.hip — cz_games_replay: G recorded games (move lists) replayed into CZ_REC_* training records in ONE launch.  No
// reference function: the reference learns from its own self-play only (main.py:1493-1554).  One lane = one game, in the frame
// of cz_posframe.h: a wave owns a group of 64 games, stages their start boards once, and every lane keeps ITS board as 23
// packed words in registers across all plies of its game — czg_step (cz_games.h) lists the position's moves with czm_list or
// czk_position, finds the given move in the list and makes it on the words; no board goes back to memory between plies.
// Per ply the wave's 64 records are assembled in LDS, one row of CZG_ROW words per lane (153 = 152 + 1: the 64 lanes' dword
// and halfword stores at the same offset of their rows fall on different banks), and leave as 16-byte stores, 38 contiguous
// pieces per record, consecutive lanes on consecutive pieces of one record.  The generators' scratch has its own 8.5 KB beside
// the rows (czk_position reads it while it puts the list).  A wave runs until its longest game is over: a lane whose game has
// ended or stopped runs along on an empty board (czg_step's go = false) and, while its game still has plies given, writes
// their records as zeros.  The host sorts the games by length, so that a wave's games end together; rec_offset puts the
// records back where the caller wants them.  49.0 KB of LDS per wave: three waves per CU.
#include "cz_games_body.h"

static_assert(CZG_OK == CZ_GAME_OK && CZG_ILLEGAL == CZ_GAME_ILLEGAL && CZG_AFTER_END == CZ_GAME_AFTER_END && CZG_BAD_BOARD == CZ_GAME_BAD_BOARD &&
              CZG_BAD_LEN == CZ_GAME_BAD_LEN && CZG_RED_KING_GONE == CZ_GAME_RED_KING_GONE && CZG_BLACK_KING_GONE == CZ_GAME_BLACK_KING_GONE,
              "cz_games.h restates include/cchess_hip.h");
static_assert(CZ_REC_BYTES == 608 && CZ_REC_SIDE == 90 && CZ_REC_COUNT == 91 && CZ_REC_Z == 92 && CZ_REC_PLY == 94 && CZ_REC_LABELS == 96 &&
              CZ_REC_VISITS == 352, "the record layout k_games_replay writes word by word");

namespace {

// the body is czg_replay_body (cz_games_body.h), shared with k_games_read (cz_notation.hip); here a move is a uint16 label
template <int RULES>
__global__ __launch_bounds__(64) void k_games_replay(const CzmTables *__restrict__ gtab, const uint16_t *__restrict__ srcdst,
                                                     const uint8_t *__restrict__ start_boards, const uint8_t *__restrict__ start_side,
                                                     const uint16_t *__restrict__ moves, int stride, const int32_t *__restrict__ len,
                                                     const int8_t *__restrict__ result, int G, const int32_t *__restrict__ rec_offset, int total,
                                                     uint8_t *__restrict__ records, int32_t *__restrict__ valid, uint8_t *__restrict__ status,
                                                     uint8_t *__restrict__ end_flags, uint8_t *__restrict__ final_boards, uint8_t *__restrict__ final_side) {
    czg_replay_body<RULES, uint16_t>(gtab, srcdst, nullptr, start_boards, start_side, moves, stride, len, result, G, rec_offset, total, records, valid,
                                     status, end_flags, final_boards, final_side, nullptr);
}

}  // namespace

int cz_games_replay(cz_ctx *c, const uint8_t *start_boards, const uint8_t *start_side, const uint16_t *moves, int stride, const int32_t *len,
                    const int8_t *result, int G, int rules, const int32_t *rec_offset, int total, uint8_t *records, int32_t *valid,
                    uint8_t *status, uint8_t *end_flags, uint8_t *final_boards, uint8_t *final_side) {
    CZ_REQUIRE(c && G >= 0, "cz_games_replay: null ctx / negative G");
    CZ_REQUIRE(stride >= 0 && stride <= 65535 && total >= 0, "cz_games_replay: 0 <= stride <= 65535 and total >= 0 required");
    CZ_REQUIRE(rules == 0 || rules == 1, "cz_games_replay: rules is 0 (capture) or 1 (king-safe)");
    if (G == 0) return CZ_OK;
    CZ_REQUIRE(moves && len && result && rec_offset && valid && status && end_flags,
               "cz_games_replay: moves, len, result, rec_offset, valid, status, end_flags required");
    CZ_REQUIRE((reinterpret_cast<uintptr_t>(records) & 15u) == 0, "cz_games_replay: records must be 16-byte aligned");
    CZ_REQUIRE(!final_boards || final_side, "cz_games_replay: final_boards needs final_side");
    const dim3 grid(czf_persistent_grid((G + 63) / 64, 3));   // 49.0 KB of LDS per wave: three waves per CU
#define CZG_LAUNCH(R) hipLaunchKernelGGL((k_games_replay<R>), grid, dim3(64), 0, c->stream, c->mask_tab, c->tab.srcdst, start_boards, start_side, moves, stride, \
                                         len, result, G, rec_offset, total, records, valid, status, end_flags, final_boards, final_side)
    if (rules) CZG_LAUNCH(1);
    else CZG_LAUNCH(0);
#undef CZG_LAUNCH
    CZ_HIP(hipGetLastError());
    return CZ_OK;
}
