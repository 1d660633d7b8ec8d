"""cz_successors, Rules.perft / divide and arena.exhaustive_openings on the GPU.

cz_successors is held byte for byte, on all five outputs, to tests/perft_model.successors — the numpy statement of its contract
— at the smallest shapes at which its boundary logic can go wrong: G in {1, 63, 64, 65, 200} (one ragged group, one full group,
a group and one parent, several groups), king-safe lists (~40 children per parent) and pseudo-legal lists of open boards (100+
children per parent: a group's children run over many tiles), padded and CZ_MOVES_NO_PAD, parents without children at the first,
a middle and the last index of a group, groups whose child total is no multiple of 8 (their range ends inside a 16-byte piece that
the next group, another wave, shares).  Every output lies between 256 sentinel bytes that must survive the launch.
Rules.perft is held to tests/golden/perft.json, whose start-position node row is the published Xiangqi perft table."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import perft_model

pytestmark = pytest.mark.gpu

SENTINEL, FENCE = 0xA5, 256
OUTPUTS = (("boards", 90, np.uint8), ("side", 1, np.uint8), ("captured", 1, np.uint8), ("parent", 4, np.int32), ("label", 2, np.uint16))


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, "perft.json")))


@pytest.fixture(scope="module")
def pool(fixture, rules_golden):
    """the positions the batches are drawn from: the fixture's, every 40th golden position with both kings, open boards (their
    pseudo-legal lists hold 60-110 moves), and a board the generators refuse (a third rook of the side to move: no children)"""
    from conftest import open_boards
    fb = np.array([p["board"] for p in fixture["positions"]], np.uint8)
    fs = np.array([p["side"] for p in fixture["positions"]], np.uint8)
    g = rules_golden
    keep = [i for i in range(0, len(g["boards"]), 40) if (g["boards"][i] == 1).sum() == 1 and (g["boards"][i] == 8).sum() == 1]
    ob, os_ = open_boards(60, 9)
    refused = np.array(fixture["start"]["board"], np.uint8)
    refused[4 * 9 + 4] = 3
    longest = [i for i, p in enumerate(fixture["positions"]) if p["tag"] == "open"]   # 97, 103 and 97 pseudo-legal moves
    return np.concatenate([fb, ob, g["boards"][keep]]), np.concatenate([fs, os_, g["side"][keep]]), refused, longest


def _batch(pool, G):
    """G positions of the pool, open boards and game positions interleaved, the fixture's open boards among them; in every
    group of three or more parents the first, a middle and the last parent are boards the generators refuse: no children under
    either kind of list"""
    pb, ps, refused, longest = pool
    idx = (np.arange(G) * 7) % len(pb)
    if G >= 8:
        idx[1:1 + len(longest)] = longest
    boards, side = pb[idx].copy(), ps[idx].copy()
    barren = []
    for g0 in range(0, G, 64):
        n = min(64, G - g0)
        if n >= 3:
            barren += [g0, g0 + n // 2, g0 + n - 1]
    boards[barren], side[barren] = refused, 0
    return boards, side, barren


def _raw(rules, boards, side, moves, offsets, T, G=None, null=(), misalign=0):
    """cz_successors through the C ABI, every output between FENCE sentinel bytes -> (rc, {name: array}); asserts the sentinels"""
    from cchess_zero_amd._lib import lib
    from cchess_zero_amd.engine import _ptr
    rules.ctx.bind_stream()
    bufs, ptrs = {}, []
    for name, width, _ in OUTPUTS:
        if name in null:
            ptrs.append(None)
            continue
        bufs[name] = torch.full((FENCE + width * T + FENCE + 16,), SENTINEL, dtype=torch.uint8, device=rules.dev)
        assert bufs[name].data_ptr() % 16 == 0
        ptrs.append(C.c_void_p(bufs[name].data_ptr() + FENCE + (misalign if name == "boards" else 0)))
    rc = lib().cz_successors(rules.ctx.h, _ptr(boards), _ptr(side), len(boards) if G is None else G, _ptr(moves), _ptr(offsets), T, *ptrs)
    torch.cuda.synchronize()
    out = {}
    for name, width, dtype in OUTPUTS:
        if name in bufs:
            h = bufs[name].cpu().numpy()
            assert (h[:FENCE] == SENTINEL).all() and (h[FENCE + width * T:] == SENTINEL).all(), "%s: bytes outside the output were written" % name
            out[name] = h[FENCE:FENCE + width * T].view(dtype).reshape((T, 90) if name == "boards" else (T,))
    return rc, out


def _lists(rules, boards, side, kingsafe, pad):
    if kingsafe:
        mv, cnt, _, _ = rules.movegen_kingsafe(boards, side, want_mask=False, pad=pad)
    else:
        mv, cnt, _ = rules.movegen(boards, side, want_mask=False, pad=pad)
    return mv, cnt


@pytest.mark.parametrize("G", [1, 63, 64, 65, 200])
def test_successors_equal_the_model(rules, pool, G):
    boards, side, barren = _batch(pool, G)
    db, ds = torch.from_numpy(boards).to(rules.dev), torch.from_numpy(side).to(rules.dev)
    ragged = 0
    for kingsafe in (True, False):
        for pad in (True, False):
            mv, cnt = _lists(rules, db, ds, kingsafe, pad)
            hm, hc = mv.cpu().numpy().view(np.uint16), cnt.cpu().numpy().view(np.uint16)
            assert all(hc[i] == 0xFFFF for i in barren) and (hc != 0xFFFF).sum() == G - len(barren)
            want = perft_model.successors(boards, side, hm, hc)
            offsets, T = want[5], int(want[5][-1])
            if not kingsafe:
                assert G < 63 or ((hc != 0xFFFF) & (hc > 100)).any()            # 100+ children of one parent
            ragged += sum(int(offsets[min(g0 + 64, G)] - offsets[g0]) % 8 != 0 for g0 in range(0, G, 64))
            rc, got = _raw(rules, db, ds, mv, torch.from_numpy(offsets).to(rules.dev), T)
            assert rc == 0
            for (name, _, _), w in zip(OUTPUTS, want):
                assert np.array_equal(got[name], w), (G, kingsafe, pad, name, np.nonzero(got[name] != w)[0][:5])
            # the public call: the same children from the same lists
            pub = rules.successors(db, ds, mv, cnt)
            for t, w, dt in zip(pub, want, (np.uint8, np.uint8, np.uint8, np.int32, np.uint16)):
                assert np.array_equal(t.cpu().numpy().view(dt), w)
    assert ragged > 0   # some group's range ended inside a 16-byte piece


def test_successors_null_outputs_alignment_and_empty_batches(rules, pool):
    from cchess_zero_amd._lib import CchessHipError, check
    boards, side, _ = _batch(pool, 65)
    db, ds = torch.from_numpy(boards).to(rules.dev), torch.from_numpy(side).to(rules.dev)
    mv, cnt = _lists(rules, db, ds, True, False)
    want = perft_model.successors(boards, side, mv.cpu().numpy().view(np.uint16), cnt.cpu().numpy().view(np.uint16))
    off, T = torch.from_numpy(want[5]).to(rules.dev), int(want[5][-1])
    for null in (("side",), ("captured",), ("parent",), ("label",), ("side", "captured", "parent", "label")):
        rc, got = _raw(rules, db, ds, mv, off, T, null=null)
        assert rc == 0 and set(got) == {n for n, _, _ in OUTPUTS} - set(null)
        for (name, _, _), w in zip(OUTPUTS, want):
            assert name in null or np.array_equal(got[name], w), (null, name)
    for misalign in (2, 8):   # out_boards off a 16-byte line: refused, nothing written
        rc, got = _raw(rules, db, ds, mv, off, T, misalign=misalign)
        assert rc != 0 and all((a.view(np.uint8) == SENTINEL).all() for a in got.values())
        with pytest.raises(CchessHipError, match="16-byte aligned"):
            check(rc, "cz_successors")
    for G, total in ((0, 0), (0, T), (65, 0)):   # no launch
        rc, got = _raw(rules, db, ds, mv, off, total, G=G)
        assert rc == 0


def _rows(entry, depth):
    return {k: entry[k][:depth + 1] for k in ("nodes", "captures", "checks", "mates")}


def _as_lists(t, i=0, depth=None):
    return {k: [int(x) for x in v[i][:None if depth is None else depth + 1]] for k, v in t.items()}


def test_perft_start_position_depth_5_with_stats(rules, fixture):
    s = fixture["start"]
    assert _as_lists(rules.perft(s["board"], [s["side"]], 5, stats=True)) == _rows(s, 5)
    assert _as_lists(rules.perft(s["board"], [s["side"]], 5)) == {"nodes": s["nodes"]}   # the last ply counted, not made


def test_perft_every_fixture_position_in_one_call_and_one_by_one(rules, fixture):
    P = [fixture["start"]] + fixture["positions"]
    boards, side = np.array([p["board"] for p in P], np.uint8), np.array([p["side"] for p in P], np.uint8)
    for stats in (True, False):
        one = rules.perft(boards, side, 3, stats=stats)
        assert all(v.shape == (len(P), 4) and v.dtype == np.int64 for v in one.values())
        for i, p in enumerate(P):
            d = min(p["depth"], 3)
            want = _rows(p, d) if stats else {"nodes": p["nodes"][:d + 1]}
            assert _as_lists(one, i, d) == want, (p.get("source", "start"), stats)
            assert _as_lists(rules.perft(boards[i], side[i:i + 1], 3, stats=stats)) == _as_lists(one, i), (i, stats)
            if p["depth"] < 3:   # to its own depth too: the last ply is then another one
                assert _as_lists(rules.perft(boards[i], side[i:i + 1], p["depth"], stats=stats)) == want, (i, stats)


def test_perft_refuses_a_root_the_generators_refuse(rules, pool):
    from cchess_zero_amd._lib import CchessHipError
    for stats in (False, True):
        for depth in (0, 1, 2):
            with pytest.raises(CchessHipError, match="not a Xiangqi set"):
                rules.perft(np.stack([pool[0][0], pool[2]]), [int(pool[1][0]), 0], depth, stats=stats)


def test_perft_chunking_and_divide(rules, fixture):
    s = fixture["start"]
    for stats in (False, True):
        whole4, whole3 = rules.perft(s["board"], [0], 4, stats=stats), rules.perft(s["board"], [0], 3, stats=stats)
        assert _as_lists(whole4) == (_rows(s, 4) if stats else {"nodes": s["nodes"][:5]})
        assert _as_lists(rules.perft(s["board"], [0], 4, stats=stats, chunk=4096)) == _as_lists(whole4)
        assert _as_lists(rules.perft(s["board"], [0], 3, stats=stats, chunk=1)) == _as_lists(whole3)
    div = rules.divide(s["board"], 0, 4)
    assert len(div) == 44 and sum(div.values()) == 3290240
    assert all(len(k) == 4 and k[0] in "abcdefghi" and k[2] in "abcdefghi" for k in div)
    div1 = rules.divide(s["board"], 0, 1)
    assert list(div1) == list(div) and set(div1.values()) == {1}


def test_perft_start_position_depth_6(rules, fixture):
    """5 392 831 844: the sixth number of the published table, the last ply counted on the 133 M positions of depth 5."""
    s = fixture["start"]
    nodes = rules.perft(s["board"], [0], 6)["nodes"][0]
    assert [int(x) for x in nodes] == s["nodes"] + [s["nodes_depth6"]] and int(nodes[6]) == 5392831844


def test_exhaustive_openings(rules):
    from cchess_zero_amd.arena import exhaustive_openings
    from cchess_zero_amd.rules import START_BOARD
    op = exhaustive_openings(2)
    assert len(op) == 1920 and len(set(int(k) for k in op.keys)) == 1920 and (op.side == 0).all()
    assert np.array_equal(rules.hash(op.boards, op.side).cpu().numpy().view(np.uint64), op.keys)
    assert ((op.boards == 1).sum(axis=1) == 1).all() and ((op.boards == 8).sum(axis=1) == 1).all()
    # every line replays from the start board to its board, and rr counts the plies since the last capture
    boards = torch.from_numpy(np.tile(START_BOARD, (len(op), 1))).to(rules.dev)
    side = torch.zeros(len(op), dtype=torch.uint8, device=rules.dev)
    lines = np.array(op.moves, np.int64)
    assert lines.shape == (1920, 2)
    rr = np.zeros(len(op), np.int32)
    for ply in range(2):
        cap, term = rules.apply_move(boards, side, torch.from_numpy(lines[:, ply].astype(np.uint16).view(np.int16)).to(rules.dev))
        assert not term.any()
        rr = np.where(cap.cpu().numpy() != 0, 0, rr + 1)
    assert np.array_equal(boards.cpu().numpy(), op.boards) and np.array_equal(side.cpu().numpy(), op.side) and np.array_equal(rr, op.rr)
    op3 = exhaustive_openings(3)
    assert 44 < len(op3) < 79666 and len(set(int(k) for k in op3.keys)) == len(op3) and (op3.side == 1).all()   # transpositions exist
    assert all(len(m) == 3 for m in op3.moves)
