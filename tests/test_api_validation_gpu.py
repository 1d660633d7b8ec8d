"""Argument checks of the rules, search and self-play entry points on a live context: each call below is refused before
any launch with CZ_EINVAL and a text that names the entry point, the G = 0 forms are no-ops, and the context works afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _refused(ctx, name, *args):
    from cchess_zero_amd._lib import CchessHipError
    with pytest.raises(CchessHipError) as e:
        ctx.call(name, *args)
    text = str(e.value).split("): ", 1)[1]         # "<name> failed (<rc>): <cz_last_error()>"
    assert "(-1)" in str(e.value) and text.startswith(name + ":"), str(e.value)


def _off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


def test_bad_arguments_are_refused_before_any_launch():
    from cchess_zero_amd import _lib
    from cchess_zero_amd.engine import Context
    from cchess_zero_amd.rules import START_BOARD
    G = 2
    ctx, fresh = Context(G, 64), Context(G, 64)    # fresh: never reset
    dev = ctx.device

    def z(shape, dtype):
        return torch.zeros(shape, dtype=dtype, device=dev)
    boards = torch.from_numpy(np.tile(START_BOARD, (G, 1)).astype(np.uint8)).to(dev)
    side = z(G, torch.uint8)
    moves, count, mask = z((G + 1, 128), torch.int16), z(G, torch.int16), z((G, 66), torch.int32)
    i32, u8, keys = z(G, torch.int32), z(G, torch.uint8), z((G, 8), torch.int64)
    planes = z((G, 90, 64), torch.float32)

    # rules
    _refused(ctx, "cz_movegen_ex", boards, side, G, moves, count, None, 2)
    _refused(ctx, "cz_movegen", boards, side, G, _off(moves, 2), count, None)
    _refused(ctx, "cz_movegen_kingsafe", boards, side, G, None, None, None, None, 0)
    for stride, fold in ((8, 1), (8, 9), (0, 3)):
        _refused(ctx, "cz_repetition", keys, z((G, 8), torch.uint8), stride, i32, None, side, G, fold, u8, None)
    _refused(ctx, "cz_threats", boards, side, G, _off(z(G * 4 + 1, torch.int64), 4))
    for dtype, channels in ((7, 14), (_lib.F32, 13), (_lib.F32, 65)):
        _refused(ctx, "cz_encode_planes", boards, side, G, planes, dtype, channels, 0)
    for temperature in (0.0, NAN):
        _refused(ctx, "cz_records_expand", z(_lib.REC_BYTES, torch.uint8), 1, None, temperature, z(90 * 14, torch.float32),
                 z(_lib.NLABELS, torch.float32), z(1, torch.float32))
    for stride, rules in ((4, 2), (65536, 0)):
        _refused(ctx, "cz_games_replay", None, None, z((G, 4), torch.int16), stride, i32, z(G, torch.int8), G, rules, i32, 0, None,
                 z(G, torch.int32), u8, z(G, torch.uint8), None, None)

    # search
    for g in (0, 3):
        _refused(ctx, "cz_search_reset", boards, side, None, g)
    ctx.call("cz_search_reset", boards, side, None, G)
    need = z(G, torch.uint8)
    _refused(fresh, "cz_search_select", 1, None, planes, _lib.F32, 14, need)
    _refused(ctx, "cz_search_select", 2, None, planes, _lib.F32, 14, need)
    _refused(ctx, "cz_search_select_compact", 2, None, planes, _lib.F32, 14, None, None)
    _refused(ctx, "cz_search_select_k", 1, 2, None, planes, _lib.F32, 14, need)
    for width in (0, 65):
        _refused(ctx, "cz_search_set_width", width)
    _refused(ctx, "cz_search_set_terminal_extra", 65)

    # self-play
    _refused(fresh, "cz_selfplay_begin", 4, None, None, None)
    for max_plies in (0, 65536):
        _refused(ctx, "cz_selfplay_begin", max_plies, None, None, None)
    _refused(ctx, "cz_selfplay_begin", 4, boards, None, None)
    _refused(ctx, "cz_selfplay_set_rules", 1)
    ctx.call("cz_selfplay_begin", 4, None, None, None)
    u, played = z(G, torch.float32), z(G, torch.int16)
    for temperature, eps, min_sims in ((0.0, 0.25, 0), (1.0, 2.0, 0), (1.0, 0.25, -1)):
        _refused(ctx, "cz_selfplay_choose", None, u, None, temperature, C.c_float(eps), min_sims, played)

    # nothing to do is no error
    assert ctx.call("cz_movegen", None, None, 0, None, None, None) == 0
    assert ctx.call("cz_hash", None, None, 0, None) == 0
    assert ctx.call("cz_apply_move", None, None, None, 0, None, None, None) == 0
    assert ctx.call("cz_successors", None, None, 0, None, None, 0, None, None, None, None, None) == 0

    # and the context still works
    ctx.call("cz_movegen", boards, side, G, moves, count, mask)
    status, nodes = z(G, torch.int32) - 1, z(G, torch.int32) - 1
    ctx.call("cz_search_status", status, nodes, None, None)
    ctx.synchronize()
    assert count.cpu().tolist() == [44, 44] and status.cpu().tolist() == [0, 0] and nodes.cpu().tolist() == [1, 1]
    assert (moves[:G, :44].cpu().numpy().view(np.uint16) < _lib.NLABELS).all() and int(moves[G].abs().sum()) == 0
    for c in (ctx, fresh):
        c.close()
