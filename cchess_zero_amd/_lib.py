"""ctypes binding of libcchess_hip.so (C-ABI: include/cchess_hip.h).

There is NO CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CCHESS_HIP_LIB: another build of the SAME library (same-box A/B of kernel changes, tools/ab_lib.sh); default: in-tree
LIB_PATH = os.environ.get("CCHESS_HIP_LIB") or os.path.join(_HERE, "libcchess_hip.so")

NLABELS = 2086
MAXMOVES = 128
NSQ = 90
MASK_WORDS = 66
F32, BF16, F16 = 0, 1, 2
# one packed self-play record (include/cchess_hip.h: CZ_REC_*)
REC_BYTES, REC_SIDE, REC_COUNT, REC_Z, REC_FLAGS, REC_PLY, REC_LABELS, REC_VISITS = 608, 90, 91, 92, 93, 94, 96, 352
# the self-play counters, getter by getter, in the order of the library's one array (csrc/cz_internal.h: CzSpSlot)
SP_STATS = ("games", "red_wins", "black_wins", "draws", "plies", "stalled", "dropped", "sims")
SP_RULES_STATS = ("mates", "repetitions", "perpetuals")   # cz_selfplay_rules_stats
SP_CHASE_STATS = ("chases",)                               # cz_selfplay_chase_stats
SP_AVOID_STATS = ("avoided", "forced_repetitions")         # cz_selfplay_avoid_stats
SP_TABLEBASE_STATS = ("tablebase",)                        # cz_selfplay_tablebase_stats
SP_RESIGN_STATS = ("resigned", "playon_games", "playon_would_resign", "playon_false_positives")   # cz_selfplay_resign_stats
# why a match game ended (include/cchess_hip.h: CZ_MATCH_*); 0 = not finished
MATCH_KING, MATCH_RR60, MATCH_PLY_CAP, MATCH_ABORTED, MATCH_MATE, MATCH_REPETITION, MATCH_PERPETUAL = 1, 2, 3, 4, 5, 6, 7
MATCH_CHASE = 9   # 8 is not assigned
MATCH_RESIGN = 10
MATCH_TABLEBASE = 11   # cz_match_set_tablebase / cz_selfplay_set_tablebase: the position after the move is in a table
# verdicts of cz_repetition (include/cchess_hip.h: CZ_REP_*)
REP_NONE, REP_DRAW, REP_RED_LOSES, REP_BLACK_LOSES = 0, 1, 2, 3
# why cz_repetition_chase gave its verdict (include/cchess_hip.h: CZ_CAUSE_*)
CAUSE_NONE, CAUSE_CHECK, CAUSE_CHASE = 0, 1, 2
# summary bits of cz_repetition_moves (include/cchess_hip.h: CZ_REPMOVES_*)
REPMOVES_REMOVED, REPMOVES_FORCED, REPMOVES_OPP_LOSES = 1, 2, 4
# position flags of cz_movegen_kingsafe (include/cchess_hip.h: CZ_POS_*)
POS_IN_CHECK, POS_CAN_TAKE_KING, POS_NO_SAFE_MOVE = 1, 2, 4
MATE_NONE = 0x7FFF   # cz_mate_backup (include/cchess_hip.h: CZ_MATE_NONE): no mate proven
TB_ILLEGAL, TB_UNKNOWN, TB_MISS, TB_MAX_SLOTS = -32768, 32767, 32766, 10   # tablebase values (include/cchess_hip.h: CZ_TB_*)
TB_SET_MAX = 256   # signatures of one table set (CZ_TB_SET_MAX)

# cz_games_replay (include/cchess_hip.h: CZ_GAME_*): why a game's replay stopped, and the end_flags bits beside POS_*
GAME_OK, GAME_ILLEGAL, GAME_AFTER_END, GAME_BAD_BOARD, GAME_BAD_LEN, GAME_AMBIGUOUS = 0, 1, 2, 3, 4, 5   # 5: cz_games_read only
GAME_STATUS = ("ok", "illegal", "after_end", "bad_board", "bad_len", "ambiguous")
GAME_RED_KING_GONE, GAME_BLACK_KING_GONE = 16, 32

_u8p, _u16p, _i32p, _f32p, _vp = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p

_SIGS = {
    "cz_last_error": (C.c_char_p, []),
    "cz_version": (C.c_int, []),
    "cz_crc32c": (C.c_uint, [C.c_char_p, C.c_size_t]),
    "cz_tables": (C.c_int, [C.POINTER(C.c_void_p)] * 4),
    "cz_mirror_table": (C.c_int, [C.POINTER(C.c_void_p)]),
    "cz_zobrist": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "cz_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "cz_destroy": (None, [C.c_void_p]),
    "cz_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cz_synchronize": (C.c_int, [C.c_void_p]),
    "cz_malloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "cz_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cz_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "cz_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "cz_movegen": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _u16p, _u16p, _vp]),
    "cz_movegen_ex": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _u16p, _u16p, _vp, C.c_int]),
    "cz_movegen_kingsafe": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _u16p, _u16p, _vp, _u8p, C.c_int]),
    "cz_movegen_checks": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _u16p, _u16p, _u8p, C.c_int]),
    "cz_mate_backup": (C.c_int, [C.c_void_p, _i32p, C.c_int, C.c_int, _vp, _u16p, _u16p, C.c_int, C.c_int, _vp, _u16p]),
    "cz_tb_entries": (C.c_int, [C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]),
    "cz_tb_pass": (C.c_int, [C.c_void_p, C.c_char_p, _vp, C.POINTER(C.c_void_p), C.c_int, _vp]),
    "cz_tb_probe": (C.c_int, [C.c_void_p, C.c_char_p, _vp, _u8p, _u8p, C.c_int, _vp, _i32p]),
    "cz_tb_boards": (C.c_int, [C.c_void_p, C.c_char_p, _i32p, C.c_int, _u8p, _u8p]),
    "cz_tb_set_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "cz_tb_set_destroy": (C.c_int, [C.c_void_p]),
    "cz_tb_set_probe": (C.c_int, [C.c_void_p, C.c_void_p, _u8p, _u8p, C.c_int, _vp, _i32p]),
    "cz_book_keys": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _vp, _u8p]),
    "cz_book_entries": (C.c_int, [C.c_void_p, _u8p, C.c_int, C.c_int, _vp, _u16p, _u8p]),
    "cz_book_probe": (C.c_int, [C.c_void_p, C.c_int, _vp, _u8p, _u8p, C.c_int, _i32p, _i32p, _u8p]),
    "cz_book_choose": (C.c_int, [C.c_void_p, C.c_int, _vp, _u16p, _vp, _u8p, _u8p, _vp, C.c_int, C.c_int, C.c_int, _vp, _u16p, _i32p]),
    "cz_repetition": (C.c_int, [C.c_void_p, _vp, _u8p, C.c_int, _i32p, _i32p, _u8p, C.c_int, C.c_int, _u8p, _i32p]),
    "cz_threats": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _vp]),
    "cz_repetition_chase": (C.c_int, [C.c_void_p, _vp, _u8p, _vp, C.c_int, _i32p, _i32p, _u8p, C.c_int, C.c_int, _u8p, _i32p, _u8p]),
    "cz_repetition_moves": (C.c_int, [C.c_void_p, _u8p, _u8p, _vp, _u8p, _vp, C.c_int, _i32p, _i32p, C.c_int, C.c_int, _u16p, _u16p, _u8p, _u16p, _u8p,
                                     _vp, _u8p]),
    "cz_apply_move": (C.c_int, [C.c_void_p, _u8p, _u8p, _u16p, C.c_int, _vp, _u8p, _vp]),
    "cz_successors": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _u16p, _i32p, C.c_int, _u8p, _u8p, _u8p, _i32p, _u16p]),
    "cz_hash": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _vp]),
    "cz_encode_planes": (C.c_int, [C.c_void_p, _u8p, _u8p, C.c_int, _vp, C.c_int, C.c_int, C.c_int]),
    "cz_records_expand": (C.c_int, [C.c_void_p, _u8p, C.c_int, _u8p, C.c_double, _f32p, _f32p, _f32p]),
    "cz_games_replay": (C.c_int, [C.c_void_p, _u8p, _u8p, _u16p, C.c_int, _i32p, _vp, C.c_int, C.c_int, _i32p, C.c_int, _u8p, _i32p, _u8p, _u8p, _u8p, _u8p]),
    "cz_games_read": (C.c_int, [C.c_void_p, _u8p, _u8p, _vp, C.c_int, _i32p, _vp, C.c_int, C.c_int, _i32p, C.c_int, _u8p, _i32p, _u8p, _u8p, _u8p, _u8p, _u16p]),
    "cz_search_reset": (C.c_int, [C.c_void_p, _u8p, _u8p, _i32p, C.c_int]),
    "cz_search_set_eval_cache": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_eval_cache_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "cz_search_eval_cache_collisions": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "cz_search_debug_eval_cache_key_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_debug_advance_in_global_memory": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_debug_xcache_dump": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "cz_search_debug_eval_cache_dump": (C.c_int, [C.c_void_p, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    "cz_search_set_xcache": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_xcache_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "cz_search_xcache_stats5": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "cz_search_reload": (C.c_int, [C.c_void_p, _u8p, _u8p, _u8p, _i32p]),
    "cz_search_select": (C.c_int, [C.c_void_p, C.c_int, _u8p, _vp, C.c_int, C.c_int, _u8p]),
    "cz_search_expand_backup": (C.c_int, [C.c_void_p, _vp, _vp, C.c_int]),
    "cz_search_expand_backup_fc": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, C.c_int]),
    "cz_search_select_compact": (C.c_int, [C.c_void_p, C.c_int, _vp, _vp, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "cz_set_batch_count": (C.c_int, [C.c_void_p, _vp]),
    "cz_probe_mfma_peak": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "cz_set_clock_probe": (C.c_int, [C.c_void_p, _vp, C.c_int]),
    "cz_clock_probe_last_grid": (C.c_int, [C.c_void_p]),
    "cz_search_eval_totals": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]),
    "cz_search_set_width": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_set_sim_target": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_set_terminal_extra": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_search_select_k": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _u8p, _vp, C.c_int, C.c_int, _u8p]),
    "cz_search_expand_backup_k": (C.c_int, [C.c_void_p, C.c_int, _vp, _vp, C.c_int]),
    "cz_search_root_stats": (C.c_int, [C.c_void_p, _u16p, _i32p, _f32p, _f32p, _f32p, _u16p]),
    "cz_search_lines": (C.c_int, [C.c_void_p, _vp, C.c_int, C.c_int, _u16p, _i32p, _f32p, _u16p]),
    "cz_search_advance": (C.c_int, [C.c_void_p, _u16p]),
    "cz_search_pick_ready": (C.c_int, [C.c_void_p, _i32p, C.c_int, _u16p, _u8p, _vp]),
    "cz_search_reload_finished": (C.c_int, [C.c_void_p, _u8p, _u16p, _u8p, _u8p, _i32p, _vp]),
    "cz_search_status": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p, _i32p]),
    "cz_search_root_state": (C.c_int, [C.c_void_p, _u8p, _u8p, _i32p]),
    "cz_search_tree_dump": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "cz_selfplay_begin": (C.c_int, [C.c_void_p, C.c_int, _u8p, _u8p, _i32p]),
    "cz_selfplay_active": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cz_selfplay_choose": (C.c_int, [C.c_void_p, _f32p, _f32p, _u16p, C.c_double, C.c_float, C.c_int, _u16p]),
    "cz_selfplay_adjudicate": (C.c_int, [C.c_void_p, C.c_int, _u16p, _i32p]),
    "cz_selfplay_flush": (C.c_int, [C.c_void_p, _i32p, _vp, _u8p, C.c_longlong, _vp]),
    "cz_selfplay_stats": (C.c_int, [C.c_void_p, _vp]),
    "cz_selfplay_set_rules": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_selfplay_set_repetition": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_selfplay_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "cz_selfplay_rules_stats": (C.c_int, [C.c_void_p, _vp]),
    "cz_selfplay_set_chase": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_selfplay_chase_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cz_selfplay_chase_stats": (C.c_int, [C.c_void_p, _vp]),
    "cz_selfplay_set_resign": (C.c_int, [C.c_void_p, C.c_float, C.c_int, C.c_double, C.c_ulonglong]),
    "cz_selfplay_resign_stats": (C.c_int, [C.c_void_p, _vp, _vp]),
    "cz_selfplay_set_tablebase": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cz_selfplay_tablebase_stats": (C.c_int, [C.c_void_p, _vp]),
    "cz_match_set_tablebase": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cz_match_set_resign": (C.c_int, [C.c_void_p, C.c_float, C.c_int]),
    "cz_match_create": (C.c_int, [C.c_void_p, C.c_void_p, _u8p, _u8p, _i32p, C.c_int, C.c_longlong, C.c_longlong, C.c_int,
                                  C.POINTER(C.c_void_p)]),
    "cz_match_destroy": (None, [C.c_void_p]),
    "cz_match_set_rules": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_match_set_repetition": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_match_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "cz_match_set_chase": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_match_set_avoid": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_match_avoid_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cz_selfplay_set_avoid": (C.c_int, [C.c_void_p, C.c_int]),
    "cz_selfplay_avoid_stats": (C.c_int, [C.c_void_p, _vp]),
    "cz_match_chase_history": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cz_match_active": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "cz_match_choose": (C.c_int, [C.c_void_p, C.c_int, C.c_ulonglong, _u16p]),
    "cz_match_adjudicate": (C.c_int, [C.c_void_p, _u16p]),
    "cz_match_results": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 6),
    "cz_match_finished": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_ulonglong)]),
    "cz_conv3x3_c128_bf16": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]),
    "cz_tower_c128_bf16": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, C.c_int, C.c_int]),
    "cz_net_trunk_bf16": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]),
    "cz_net_trunk_f16": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]),
    "cz_net_trunk_split": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int]),
    "cz_net_trunk_mx": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]),
    "cz_fc_heads_f32": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int]),
    "cz_tower_heads_c128_bf16": (C.c_int, [C.c_void_p, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int]),
}

EXPORTS = tuple(sorted(_SIGS))
_lib = None


class CchessHipError(RuntimeError):
    pass


def lib():
    """Loads libcchess_hip.so (built by `python -m cchess_zero_amd.build` / __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CchessHipError(
                "libcchess_hip.so is missing at %s — build it with __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path." % LIB_PATH)
        # libcchess_hip.so must share ONE HIP runtime with PyTorch (device memory and streams are
        # torch's): import torch first so that its bundled libamdhip64 is the one already mapped.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().cz_last_error()
        raise CchessHipError("%s failed (%d): %s" % (what or "cchess_hip call", rc, msg.decode() if msg else "?"))


def _ptr(t):
    """tensor -> c_void_p for a direct lib() call (tests, tools); None and a raw device pointer pass through."""
    if t is None or isinstance(t, C.c_void_p):
        return t
    return C.c_void_p(t.data_ptr())


def call(name, *args):
    """lib().<name>(*args): anything with a data_ptr() (a tensor) goes as that address, None / ctypes objects / Python scalars
    as they are.  Raises CchessHipError on a negative return, else returns the value (0, or the count a dump hands back)."""
    rc = getattr(lib(), name)(*[a.data_ptr() if hasattr(a, "data_ptr") else a for a in args])
    if rc < 0:
        check(rc, name)
    return rc


def out_pointers(name, handle, n, *args):
    """The n device pointers the getter <name>(handle, *args, &p0 .. &p[n-1]) hands back, as c_void_p."""
    ptrs = [C.c_void_p() for _ in range(n)]
    call(name, handle, *args, *[C.byref(p) for p in ptrs])
    return ptrs


_tables = None


def tables():
    """Host copies of the static tables: dict(lut[90,90] i16, unflip[2086] i16, mirror[2086] i16 — the label of the move mirrored
    across the e-file —, labels[2086] str, srcdst[2086] u16)."""
    global _tables
    if _tables is None:
        p = [C.c_void_p() for _ in range(4)]
        call("cz_tables", *[C.byref(x) for x in p])
        lut = np.ctypeslib.as_array(C.cast(p[0], C.POINTER(C.c_int16)), shape=(NSQ * NSQ,)).reshape(NSQ, NSQ).copy()
        unflip = np.ctypeslib.as_array(C.cast(p[1], C.POINTER(C.c_int16)), shape=(NLABELS,)).copy()
        raw = C.string_at(p[2], NLABELS * 5)
        labels = [raw[i * 5:i * 5 + 4].decode() for i in range(NLABELS)]
        srcdst = np.ctypeslib.as_array(C.cast(p[3], C.POINTER(C.c_uint16)), shape=(NLABELS,)).copy()
        mp = C.c_void_p()
        call("cz_mirror_table", C.byref(mp))
        mirror = np.ctypeslib.as_array(C.cast(mp, C.POINTER(C.c_int16)), shape=(NLABELS,)).copy()
        zk = C.c_void_p()
        sk = C.c_uint64()
        call("cz_zobrist", C.byref(zk), C.byref(sk))
        zob = np.ctypeslib.as_array(C.cast(zk, C.POINTER(C.c_uint64)), shape=(15 * NSQ,)).reshape(15, NSQ).copy()
        _tables = dict(lut=lut, unflip=unflip, mirror=mirror, labels=labels, srcdst=srcdst, zobrist=zob, zobrist_side=int(sk.value),
                       label2i={s: i for i, s in enumerate(labels)})
    return _tables
