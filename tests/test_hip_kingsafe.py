"""cz_movegen_kingsafe (k_movegen_kingsafe around cz_kingsafe.h's czk_position) on the GPU against tests/kingsafe_model.py: the
ordered king-safe list, its count, the 2086-bit set and the position flags, bit for bit — the corpora of
tests/test_kingsafe_host_cpu.py plus 20 k random positions, padded and CZ_MOVES_NO_PAD rows, every combination of NULL
outputs, ragged batch sizes and odd byte addresses through the raw C ABI."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import kingsafe_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


@pytest.fixture(scope="module")
def golden_model(rules_golden):
    g = rules_golden
    return (g["boards"], g["side"]) + M.model_batch(g["boards"], g["side"])


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _hold_to_model(rules, boards, side, model=None):
    lists, counts, masks, flags, pseudo = model if model is not None else M.model_batch(boards, side)
    n = len(counts)
    for pad in (True, False):
        mv, cnt, mask, pf = rules.movegen_kingsafe(boards, side, pad=pad)
        mv, cnt, mask, pf = _u16(mv), _u16(cnt), mask.cpu().numpy().view(np.uint32), pf.cpu().numpy()
        assert not (cnt == 0xFFFF).any()                                   # no position of these corpora is refused
        assert np.array_equal(cnt.astype(np.int32), counts), np.nonzero(cnt.astype(np.int32) != counts)[0][:5]
        assert np.array_equal(pf, flags), np.nonzero(pf != flags)[0][:5]
        assert np.array_equal(mask, masks), np.nonzero((mask != masks).any(axis=1))[0][:5]
        for i in range(n):
            assert np.array_equal(mv[i, :counts[i]], lists[i]), (i, pad, mv[i, :counts[i]], lists[i])
            if pad:
                assert (mv[i, counts[i]:] == 0xFFFF).all(), i
    # the set alone, the list alone, the flags alone
    none, cnt, mask, pf = rules.movegen_kingsafe(boards, side, want_moves=False)
    assert none is None and np.array_equal(_u16(cnt).astype(np.int32), counts) and np.array_equal(mask.cpu().numpy().view(np.uint32), masks)
    assert np.array_equal(pf.cpu().numpy(), flags)
    mv, cnt, none, pf = rules.movegen_kingsafe(boards, side, want_mask=False)
    assert none is None and np.array_equal(_u16(cnt).astype(np.int32), counts) and np.array_equal(pf.cpu().numpy(), flags)
    assert all(np.array_equal(_u16(mv)[i, :counts[i]], lists[i]) for i in range(n))
    assert np.array_equal(rules.in_check(boards, side).cpu().numpy(), flags)
    return M.shares(counts, flags, pseudo)


def test_golden_positions(rules, golden_model):
    boards, side = golden_model[:2]
    check, differs, mated, takes = _hold_to_model(rules, boards, side, golden_model[2:])
    assert len(boards) == 4381 and check >= 500 and differs >= 1400 and mated >= 30 and takes >= 500


def test_open_boards(rules):
    from conftest import open_boards
    boards, side = open_boards(900, 12)
    check, differs, mated, takes = _hold_to_model(rules, boards, side)
    assert check >= 120 and differs >= 350 and mated >= 1 and takes >= 400


def test_random_playouts_until_a_king_falls(rules):
    boards, side = M.playout_corpus()
    check, differs, mated, _ = _hold_to_model(rules, boards, side)
    assert len(boards) >= 5000 and check >= 500 and differs >= 1500 and mated >= 10


def test_random_positions_20k(rules):
    """20 480 positions of cchess_zero_amd.rules.random_positions (both kings on the board, up to 80 plies deep)."""
    from cchess_zero_amd.rules import random_positions
    boards, side, _ = random_positions(rules, 20480, seed=31)
    check, differs, mated, _ = _hold_to_model(rules, boards.cpu().numpy(), side.cpu().numpy())
    print("random_positions: in check %d, king-safe != pseudo-legal %d, no safe move %d of 20480" % (check, differs, mated))
    assert check >= 500 and differs >= 2000         # a quarter of the shares the CPU playouts show (9 % in check, 29 % with an unsafe move)


def _raw(rules, boards, side, G, want, flags=0, off=0, sentinel=0x5A):
    """cz_movegen_kingsafe through the raw C ABI: every buffer `off` bytes behind a 16-byte boundary (moves: always aligned), two
    rows longer than the batch and pre-filled with a sentinel byte.  want = (moves, count, mask, pos_flags) booleans.
    -> the four buffers as numpy arrays (G + 2 rows), written or not."""
    from cchess_zero_amd._lib import check, lib

    def buf(nbytes, o, fill):
        t = torch.full((nbytes + 32,), fill, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        return t[o:o + nbytes]
    b = buf(G * 90, off, 0)
    b.copy_(torch.from_numpy(np.ascontiguousarray(boards, np.uint8).reshape(-1)).cuda())
    s = buf(G, off, 0)
    s.copy_(torch.from_numpy(np.ascontiguousarray(side, np.uint8)).cuda())
    outs = [buf((G + 2) * 256, 0, sentinel), buf((G + 2) * 2, off, sentinel), buf((G + 2) * 264, off, sentinel), buf(G + 2, off, sentinel)]
    p = lambda t, w: C.c_void_p(t.data_ptr()) if w else None
    rules.ctx.bind_stream()
    check(lib().cz_movegen_kingsafe(rules.ctx.h, p(b, True), p(s, True), G, *[p(t, w) for t, w in zip(outs, want)], flags), "cz_movegen_kingsafe")
    host = [t.cpu().numpy().copy() for t in outs]
    return host[0].view(np.uint16).reshape(G + 2, 128), host[1].view(np.uint16), host[2].view(np.uint32).reshape(G + 2, 66), host[3]


def test_no_pad_rows_end_at_their_last_16_byte_piece(rules, golden_model):
    boards, side, lists, counts, masks, flags, _ = golden_model
    G = len(counts)
    mv, cnt, mask, pf = _raw(rules, boards, side, G, (True, True, True, True), flags=1)
    assert np.array_equal(cnt[:G].astype(np.int32), counts) and np.array_equal(mask[:G], masks) and np.array_equal(pf[:G], flags)
    col = np.arange(128)[None, :]
    for i in range(G):
        assert np.array_equal(mv[i, :counts[i]], lists[i]), i
    untouched = col >= ((counts[:, None] + 7) // 8) * 8          # behind the last 16-byte piece of a row
    assert (mv[:G][untouched] == 0x5A5A).all() and untouched.sum() > 0.6 * mv[:G].size
    assert (mv[G:] == 0x5A5A).all() and (cnt[G:] == 0x5A5A).all() and (mask[G:] == 0x5A5A5A5A).all() and (pf[G:] == 0x5A).all()


def test_every_combination_of_null_outputs(rules, golden_model):
    """What is asked for is right, what is not stays untouched — the flags alone included; no output at all is an error."""
    from cchess_zero_amd._lib import CchessHipError
    boards, side, lists, counts, masks, flags, _ = golden_model
    G = 321
    for want in itertools.product((False, True), repeat=4):
        if not any(want):
            with pytest.raises(CchessHipError, match="no output"):
                _raw(rules, boards[:G], side[:G], G, want)
            continue
        for nopad in (0, 1):
            mv, cnt, mask, pf = _raw(rules, boards[:G], side[:G], G, want, flags=nopad)
            if want[0]:
                for i in range(G):
                    assert np.array_equal(mv[i, :counts[i]], lists[i]), (want, i)
                    assert nopad or (mv[i, counts[i]:] == 0xFFFF).all()
                assert (mv[G:] == 0x5A5A).all()
            else:
                assert (mv == 0x5A5A).all()
            assert np.array_equal(cnt[:G].astype(np.int32), counts[:G]) and (cnt[G:] == 0x5A5A).all() if want[1] else (cnt == 0x5A5A).all()
            assert np.array_equal(mask[:G], masks[:G]) and (mask[G:] == 0x5A5A5A5A).all() if want[2] else (mask == 0x5A5A5A5A).all()
            assert np.array_equal(pf[:G], flags[:G]) and (pf[G:] == 0x5A).all() if want[3] else (pf == 0x5A).all()


@pytest.mark.parametrize("G", [1, 63, 64, 65, 4097, 400011])
def test_ragged_sizes_and_odd_addresses_raw_abi(rules, golden_model, G):
    """Batch sizes around the wave's 64 positions; boards, side, count, mask and pos_flags at a 16-byte aligned, an even and an ODD
    byte address (`moves` alone must be aligned); rows beyond the batch are not touched.  400 011 positions (all four outputs and
    the flags alone, the 16-byte and the byte path of the boards) are 6 251 groups with a last one of 11, on grids of 1 536 and
    2 560 waves: every wave walks several groups, the next one prefetched."""
    boards, side, lists, counts, masks, flags, _ = golden_model
    idx = (np.arange(G) * 37) % len(counts)
    rows = np.full((len(counts), 128), 0xFFFF, np.uint16)          # a position's list with the ABI's padding behind it
    for i, l in enumerate(lists):
        rows[i, :len(l)] = l
    many = G > 100000
    for off in (0, 1) if many else (0, 2, 1, 7):
        for want in ((True, True, True, True), (False, False, False, True)) if many else ((True, True, True, True), (False, True, True, True), (False, False, False, True)):
            mv, cnt, mask, pf = _raw(rules, boards[idx], side[idx], G, want, off=off)
            assert np.array_equal(pf[:G], flags[idx]) and (pf[G:] == 0x5A).all()
            if want[1]:
                assert np.array_equal(cnt[:G].astype(np.int32), counts[idx]) and (cnt[G:] == 0x5A5A).all()
            if want[2]:
                assert np.array_equal(mask[:G], masks[idx]) and (mask[G:] == 0x5A5A5A5A).all()
            if want[0]:
                assert np.array_equal(mv[:G], rows[idx]), off
                assert (mv[G:] == 0x5A5A).all()


def test_unaligned_moves_are_refused(rules, golden_model):
    from cchess_zero_amd._lib import CchessHipError, lib
    boards, side = golden_model[:2]
    b, s = torch.from_numpy(boards[:4]).cuda(), torch.from_numpy(side[:4]).cuda()
    mv = torch.zeros(4 * 128 + 8, dtype=torch.int16, device="cuda")
    rc = lib().cz_movegen_kingsafe(rules.ctx.h, C.c_void_p(b.data_ptr()), C.c_void_p(s.data_ptr()), 4, C.c_void_p(mv.data_ptr() + 2), None, None, None, 0)
    assert rc != 0
    assert lib().cz_movegen_kingsafe(rules.ctx.h, C.c_void_p(b.data_ptr()), C.c_void_p(s.data_ptr()), 4, None, None, None, C.c_void_p(mv.data_ptr()), 2) != 0   # unknown flag


def test_a_board_that_is_not_a_xiangqi_set_answers_0xffff(rules, rules_golden):
    g = rules_golden
    bad = g["boards"][:4].copy()
    bad[2, :] = 0
    bad[2, :3] = 3 if g["side"][2] == 0 else 10               # three rooks of the side to move
    _, cnt, _, pf = rules.movegen_kingsafe(bad, g["side"][:4])
    _, cnt0, _ = rules.movegen(bad, g["side"][:4])
    assert _u16(cnt)[2] == 0xFFFF and _u16(cnt0)[2] == 0xFFFF and pf.cpu().numpy()[2] == 0
    assert (_u16(cnt)[[0, 1, 3]] != 0xFFFF).all()


def test_movegen_itself_is_unchanged(rules, rules_golden):
    """Rules.movegen on the same inputs, before and after the king-safe launches: the golden pseudo-legal lists."""
    g = rules_golden
    rules.movegen_kingsafe(g["boards"], g["side"])
    for pad in (True, False):
        moves, count, mask = rules.movegen(g["boards"], g["side"], pad=pad)
        assert np.array_equal(_u16(count), g["counts"])
        if pad:
            assert np.array_equal(_u16(moves), g["moves"])
        else:
            col = np.arange(128)[None, :] < g["counts"][:, None]
            assert np.array_equal(_u16(moves)[col], g["moves"][col])
    _, c2, m2 = rules.movegen(g["boards"], g["side"], want_moves=False)
    assert torch.equal(m2, mask) and np.array_equal(_u16(c2), g["counts"])
