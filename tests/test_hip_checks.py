"""cz_movegen_checks (k_movegen_checks around cz_kingsafe.h's czk_checks) on the GPU against tests/mate_model.checks: the ordered
list of the king-safe moves that give check, its count and the position's own flags, bit for bit — the golden positions and the
playout corpus through Rules.checks, ragged batch sizes with sentinels behind the rows through the raw C ABI, and 100 000 random
positions against the composition the kernel replaces (king-safe list -> successors -> in_check -> compaction)."""
import ctypes as C

import numpy as np
import pytest
import torch

import kingsafe_model as M
import mate_model as MM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _model(boards, side):
    lists, flags = zip(*[MM.checks(b, int(s)) for b, s in zip(boards, side)])
    return list(lists), np.array([len(l) for l in lists], np.int32), np.array(flags, np.uint8)


@pytest.fixture(scope="module")
def golden_model(rules_golden):
    g = rules_golden
    return (g["boards"], g["side"]) + _model(g["boards"], g["side"])


def _hold_to_model(rules, boards, side, model):
    lists, counts, flags = model
    for pad in (True, False):
        mv, cnt, pf = rules.checks(boards, side, pad=pad)
        mv, cnt, pf = _u16(mv), _u16(cnt), pf.cpu().numpy()
        assert not (cnt == 0xFFFF).any()
        assert np.array_equal(cnt.astype(np.int32), counts), np.nonzero(cnt.astype(np.int32) != counts)[0][:5]
        assert np.array_equal(pf, flags), np.nonzero(pf != flags)[0][:5]
        for i in range(len(counts)):
            assert np.array_equal(mv[i, :counts[i]], lists[i]), (i, pad, mv[i, :counts[i]], lists[i])
            if pad:
                assert (mv[i, counts[i]:] == 0xFFFF).all(), i
    none, cnt, pf = rules.checks(boards, side, want_moves=False)
    assert none is None and np.array_equal(_u16(cnt).astype(np.int32), counts) and np.array_equal(pf.cpu().numpy(), flags)
    _, kcnt, _, kpf = rules.movegen_kingsafe(boards, side, want_mask=False, want_moves=False)
    assert np.array_equal(kpf.cpu().numpy(), flags)                       # the flags are movegen_kingsafe's, NO_SAFE_MOVE included
    assert (_u16(kcnt).astype(np.int32) >= counts).all()


def test_golden_positions(rules, golden_model):
    boards, side = golden_model[:2]
    _hold_to_model(rules, boards, side, golden_model[2:])
    assert len(boards) == 4381 and (golden_model[3] > 0).sum() >= 800


def test_random_playouts_until_a_king_falls(rules):
    boards, side = M.playout_corpus()
    model = _model(boards, side)
    _hold_to_model(rules, boards, side, model)
    assert len(boards) >= 5000 and (model[1] > 0).sum() >= 2000


def _raw(rules, boards, side, G, want, flags=0, sentinel=0x5A):
    """cz_movegen_checks through the raw C ABI: every output two rows longer than the batch and pre-filled with a sentinel byte.
    want = (moves, count, pos_flags) booleans -> the three buffers as numpy arrays (G + 2 rows), written or not."""
    from cchess_zero_amd._lib import check, lib
    b = torch.from_numpy(np.ascontiguousarray(boards, np.uint8).reshape(-1)).cuda()
    s = torch.from_numpy(np.ascontiguousarray(side, np.uint8)).cuda()
    outs = [torch.full((n,), sentinel, dtype=torch.uint8, device="cuda") for n in ((G + 2) * 256, (G + 2) * 2, G + 2)]
    assert outs[0].data_ptr() % 16 == 0
    p = lambda t, w: C.c_void_p(t.data_ptr()) if w else None
    rules.ctx.bind_stream()
    check(lib().cz_movegen_checks(rules.ctx.h, p(b, True), p(s, True), G, *[p(t, w) for t, w in zip(outs, want)], flags), "cz_movegen_checks")
    host = [t.cpu().numpy().copy() for t in outs]
    return host[0].view(np.uint16).reshape(G + 2, 128), host[1].view(np.uint16), host[2]


@pytest.mark.parametrize("G", [1, 63, 64, 65, 130])
def test_ragged_sizes_raw_abi(rules, golden_model, G):
    """Batch sizes around the wave's 64 positions, padded and CZ_MOVES_NO_PAD, all outputs and each output alone; what is not
    asked for and the rows behind the batch keep the sentinel."""
    boards, side, lists, counts, flags = golden_model
    idx = (int(np.nonzero(counts > 0)[0][0]) + np.arange(G) * 37) % len(counts)     # the first of them has a checking move
    cn, fl = counts[idx], flags[idx]
    for want in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        for nopad in (0, 1):
            mv, cnt, pf = _raw(rules, boards[idx], side[idx], G, want, flags=nopad)
            if want[0]:
                for i in range(G):
                    assert np.array_equal(mv[i, :cn[i]], lists[idx[i]]), (G, want, nopad, i)
                    if nopad:
                        assert (mv[i, ((cn[i] + 7) // 8) * 8:] == 0x5A5A).all(), i      # nothing behind the row's last 16-byte piece
                    else:
                        assert (mv[i, cn[i]:] == 0xFFFF).all(), i
                assert (mv[G:] == 0x5A5A).all()
            else:
                assert (mv == 0x5A5A).all()
            assert np.array_equal(cnt[:G].astype(np.int32), cn) and (cnt[G:] == 0x5A5A).all() if want[1] else (cnt == 0x5A5A).all()
            assert np.array_equal(pf[:G], fl) and (pf[G:] == 0x5A).all() if want[2] else (pf == 0x5A).all()


def test_random_positions_100k_against_the_composition(rules):
    """100 000 positions of random_positions: 1 563 groups on at most 1 536 persistent waves of the list form, so some waves
    take a second group, and a ragged last group of 32.  checks == king-safe list -> successors -> in_check -> compaction."""
    from cchess_zero_amd._lib import POS_IN_CHECK
    from cchess_zero_amd.rules import random_positions
    G = 100000
    boards, side, _ = random_positions(rules, G, seed=41)
    kmv, kcnt, _, kpf = rules.movegen_kingsafe(boards, side, want_mask=False)
    cb, cs, _, par, label = rules.successors(boards, side, kmv, kcnt)
    keep = (rules.in_check(cb, cs) & POS_IN_CHECK) != 0
    par, label = par[keep].to(torch.int64), label[keep]
    count = torch.zeros(G, dtype=torch.int64, device=boards.device).index_add_(0, par, torch.ones_like(par))
    first = torch.cumsum(count, 0) - count
    rows = torch.full((G, 128), -1, dtype=torch.int16, device=boards.device)
    rows[par, torch.arange(par.numel(), device=boards.device) - first[par]] = label
    mv, cnt, pf = rules.checks(boards, side)
    assert torch.equal(cnt.to(torch.int64), count) and torch.equal(pf, kpf)
    assert torch.equal(mv, rows)
    mv2, cnt2, _ = rules.checks(boards, side, pad=False)
    live = torch.arange(128, device=boards.device)[None, :] < count[:, None]
    assert torch.equal(cnt2, cnt) and torch.equal(mv2[live], rows[live])
    print("random_positions: %d of %d positions have a checking move, %d checks" % (int((count > 0).sum()), G, int(count.sum())))
    assert int((count > 0).sum()) >= G // 10        # the CPU playouts show 44 % of the legal roots with one


def test_argument_errors(rules, golden_model):
    from cchess_zero_amd._lib import CchessHipError, lib
    boards, side = golden_model[:2]
    with pytest.raises(CchessHipError, match="no output"):
        _raw(rules, boards[:4], side[:4], 4, (False, False, False))
    with pytest.raises(CchessHipError, match="unknown flag"):
        _raw(rules, boards[:4], side[:4], 4, (True, True, True), flags=2)
    b, s = torch.from_numpy(boards[:4]).cuda(), torch.from_numpy(side[:4]).cuda()
    mv = torch.zeros(4 * 128 + 8, dtype=torch.int16, device="cuda")
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    assert lib().cz_movegen_checks(rules.ctx.h, p(b), p(s), 4, p(mv, 2), None, None, 0) != 0 and b"16-byte aligned" in lib().cz_last_error()
    assert lib().cz_movegen_checks(rules.ctx.h, p(b), p(s), -1, p(mv), None, None, 0) != 0 and b"negative G" in lib().cz_last_error()
    assert lib().cz_movegen_checks(rules.ctx.h, p(b), p(s), 0, None, None, None, 0) == 0        # an empty batch asks for nothing


def test_a_board_that_is_not_a_xiangqi_set_answers_0xffff(rules, rules_golden):
    g = rules_golden
    bad = g["boards"][:4].copy()
    bad[2, :] = 0
    bad[2, :3] = 3 if g["side"][2] == 0 else 10               # three rooks of the side to move
    _, cnt, pf = rules.checks(bad, g["side"][:4])
    assert _u16(cnt)[2] == 0xFFFF and pf.cpu().numpy()[2] == 0
    assert (_u16(cnt)[[0, 1, 3]] != 0xFFFF).all()
