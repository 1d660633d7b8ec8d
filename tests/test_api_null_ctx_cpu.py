"""Every entry point of libcchess_hip.so that checks its arguments beside its kernels (rules, search, self-play, records,
recorded games) refuses a NULL context before it touches anything else: a negative code, a text in cz_last_error(), and the
process goes on.  No GPU: the library loads without one."""
import ctypes as C

# the entry points defined in cz_rules / cz_kingsafe / cz_repetition / cz_chase / cz_successors / cz_records / cz_games /
# cz_search / cz_selfplay .hip
ENTRY_POINTS = (
    "cz_movegen", "cz_movegen_ex", "cz_apply_move", "cz_hash", "cz_encode_planes",
    "cz_movegen_kingsafe",
    "cz_repetition", "cz_repetition_chase",
    "cz_threats",
    "cz_successors",
    "cz_records_expand",
    "cz_games_replay",
    "cz_search_set_width", "cz_search_set_sim_target", "cz_search_debug_advance_in_global_memory", "cz_search_set_terminal_extra",
    "cz_search_reset", "cz_search_reload",
    "cz_search_select", "cz_search_select_k", "cz_search_select_compact",
    "cz_search_expand_backup", "cz_search_expand_backup_k", "cz_search_expand_backup_fc",
    "cz_search_root_stats", "cz_search_advance", "cz_search_pick_ready", "cz_search_reload_finished", "cz_search_status",
    "cz_search_eval_totals", "cz_search_tree_dump",
    "cz_selfplay_begin", "cz_selfplay_set_rules", "cz_selfplay_set_repetition", "cz_selfplay_set_chase", "cz_selfplay_set_resign",
    "cz_selfplay_history", "cz_selfplay_chase_history", "cz_selfplay_active",
    "cz_selfplay_stats", "cz_selfplay_rules_stats", "cz_selfplay_chase_stats", "cz_selfplay_resign_stats",
    "cz_selfplay_choose", "cz_selfplay_adjudicate", "cz_selfplay_flush",
)


def _zero(argtype):
    """NULL for a pointer, 0 for a number"""
    if argtype in (C.c_void_p, C.c_char_p) or hasattr(argtype, "contents"):
        return None
    return argtype(0)


def test_null_context_is_refused():
    import __graft_entry__
    __graft_entry__.build_hip_only()
    from cchess_zero_amd import _lib
    L = _lib.lib()
    assert len(set(ENTRY_POINTS)) == len(ENTRY_POINTS) == 46 and set(ENTRY_POINTS) <= set(_lib.EXPORTS)
    marker = b"cz_malloc: null argument"
    for name in ENTRY_POINTS:
        res, argtypes = _lib._SIGS[name]
        assert res is C.c_int and argtypes[0] is C.c_void_p, name
        # the error text is the thread's last one: leave a known one there, so that what is read below is this call's
        assert L.cz_malloc(None, 0, None) < 0 and L.cz_last_error() == marker
        rc = getattr(L, name)(*[_zero(a) for a in argtypes])
        assert rc < 0, (name, rc)
        msg = L.cz_last_error()
        assert msg and msg != marker, (name, msg)
