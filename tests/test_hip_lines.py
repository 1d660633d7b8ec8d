"""cz_search_lines on the device against tests/lines_model.py over the same trees' dumps: every comparison is exact (moves,
visits, len equal; q equal as bits)."""
import numpy as np
import pytest
import torch

import fakenet
import lines_cases
import lines_model as LM

pytestmark = pytest.mark.gpu


class _Hip:
    """The HIP SearchEngine behind the host-array interface lines_cases.run_ply drives."""

    def __init__(self, G, cap=20000, width=1):
        from cchess_zero_amd.engine import SearchEngine
        self.e = SearchEngine(G, cap, width=width)

    def reset(self, boards, side, rr):
        self.e.reset(boards, side, rr)

    def select(self, mode):
        planes, need = self.e.select(mode)
        return planes.cpu().numpy(), need.cpu().numpy()

    def expand_backup(self, logits, value):
        self.e.expand_backup(torch.from_numpy(logits).cuda(), torch.from_numpy(value).cuda())


def _model(dumps, allowed, n_lines, max_len):
    """lines_from_dump over every tree -> the four arrays stacked like lines_host's; allowed: None or [G, 66] masks."""
    per = [LM.lines_from_dump(d, None if allowed is None else LM.mask_labels(allowed[g]), n_lines, max_len) for g, d in enumerate(dumps)]
    return dict(moves=np.stack([p[0] for p in per]), visits=np.stack([p[1] for p in per]), q=np.stack([p[2] for p in per]),
                len=np.stack([p[3] for p in per]))


def _assert_equal(got, want, what):
    for k in ("moves", "visits", "len"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["q"].view(np.uint32), want["q"].view(np.uint32)), (what, "q")


def _dumps(engine):
    return [engine.tree_dump(g) for g in range(engine.G)]


def _pick_all(engine):
    """cz_search_pick_ready with every threshold at 0 (all trees ready; the trees are not touched) -> played u16 [G]."""
    thr = torch.zeros(engine.G, dtype=torch.int32, device=engine.dev)
    played = torch.empty(engine.G, dtype=torch.int16, device=engine.dev)
    ready = torch.empty(engine.G, dtype=torch.uint8, device=engine.dev)
    engine.ctx.call("cz_search_pick_ready", thr, 0, played, ready, None)
    assert bool(ready.all().item())
    return played.cpu().numpy().view(np.uint16)


@pytest.fixture(scope="module")
def plies(rules_golden):
    """64 corpus trees (fakenet pos, salt 99): two plies of 1 + 48 lock-steps with a greedy advance between them.  Per ply:
    the root positions, their king-safe masks, every tree's dump, lines_host(5, 8) without and with the masks, and the
    greedy pick of cz_search_pick_ready."""
    from cchess_zero_amd.rules import Rules
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    hip = _Hip(64)
    rules = Rules(ctx=hip.e.ctx)
    hip.reset(boards, side, rr)
    fwd = fakenet.make_forward("pos", 99)
    out = []
    for ply in range(2):
        lines_cases.run_ply(hip, fwd, 48)
        rb, rs, _ = hip.e.root_state()
        mask = rules.movegen_kingsafe(rb, rs, want_moves=False)[2]
        out.append(dict(boards=rb.cpu().numpy(), side=rs.cpu().numpy(), mask=mask.cpu().numpy(), dumps=_dumps(hip.e),
                        free=hip.e.lines_host(5, 8), safe=hip.e.lines_host(5, 8, allowed=mask), picked=_pick_all(hip.e),
                        stats=hip.e.root_stats_host()))
        hip.e.advance(lines_cases.greedy(out[-1]["stats"]))
    return out


def test_lines_match_the_model_through_an_advance(plies):
    assert int(plies[0]["side"].sum()) == 32   # half the roots are black to move
    ties = fours = wide = dropped = 0
    for ply, p in enumerate(plies):
        want_free, want_safe = _model(p["dumps"], None, 5, 8), _model(p["dumps"], p["mask"], 5, 8)
        _assert_equal(p["free"], want_free, ("free", ply))
        _assert_equal(p["safe"], want_safe, ("safe", ply))
        f = p["free"]
        ties += int(((f["len"][:, 1] > 0) & (f["visits"][:, 0, 0] == f["visits"][:, 1, 0])).sum())
        fours += int((f["len"] >= 4).sum())
        st = p["stats"]
        wide += int(((st["N"] > 0).sum(axis=1) >= 5).sum())
        for g in range(64):
            n = int(st["count"][g])
            ok = set(LM.mask_labels(p["mask"][g]))
            dropped += int(any(int(l) not in ok for l in st["label"][g, :n]))
    # not a vacuous run: a tie between the two most visited children, a line of four, five visited children, a masked child
    assert ties >= 1 and fours >= 1 and wide >= 1 and dropped >= 1
    assert any((p["free"]["moves"][:, 0, 0] != p["safe"]["moves"][:, 0, 0]).any() or (p["free"]["len"] != p["safe"]["len"]).any() for p in plies)


def test_line_zero_is_the_greedy_move(plies):
    for p in plies:
        assert (p["free"]["len"][:, 0] >= 1).all()
        assert np.array_equal(p["free"]["moves"][:, 0, 0], p["picked"])


def test_lines_replay_legally_on_the_device(plies):
    """Every move of every line is in Rules.movegen's set of the position it is played in (Rules.apply_move replays it)."""
    from cchess_zero_amd.rules import Rules
    rules = Rules()
    for p in plies:
        for key in ("free", "safe"):
            ln = p[key]
            L = ln["len"].reshape(-1).astype(np.int64)          # [64 * 5]
            mv = ln["moves"].reshape(len(L), -1)
            b = torch.from_numpy(np.repeat(p["boards"], 5, axis=0)).cuda().contiguous()
            s = torch.from_numpy(np.repeat(p["side"], 5)).cuda().contiguous()
            for i in range(int(L.max())):
                live = L > i
                mask = rules.movegen(b, s, want_moves=False)[2].cpu().numpy().view(np.uint32)
                m = mv[:, i].astype(np.int64)
                m_ok = np.where(live, m, 0)
                bit = (mask[np.arange(len(L)), m_ok >> 5] >> (m_ok & 31).astype(np.uint32)) & 1
                assert bit[live].all(), (key, i)
                labels = np.where(live, mv[:, i], 0xFFFF).astype(np.uint16)
                rules.apply_move(b, s, labels)
                if key == "safe" and i == 0:   # the first move of a masked line is king-safe
                    own = np.repeat(p["mask"].view(np.uint32), 5, axis=0)
                    assert ((own[np.arange(len(L)), m_ok >> 5] >> (m_ok & 31).astype(np.uint32)) & 1)[live].all()


def test_long_lines_and_truncation(rules_golden):
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    hip = _Hip(8)
    hip.reset(boards[:8], side[:8], rr[:8])
    lines_cases.run_ply(hip, fakenet.make_forward("deep", 913), 96)
    dumps = _dumps(hip.e)
    full, cut = hip.e.lines_host(3, 64), hip.e.lines_host(3, 16)
    _assert_equal(full, _model(dumps, None, 3, 64), "max_len 64")
    _assert_equal(cut, _model(dumps, None, 3, 16), "max_len 16")
    assert int(full["len"].max()) >= 20 and int(cut["len"].max()) == 16


@pytest.fixture(scope="module")
def small(rules_golden):
    """Three corpus trees after 1 + 24 lock-steps, and their dumps."""
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    hip = _Hip(3)
    hip.reset(boards[:3], side[:3], rr[:3])
    lines_cases.run_ply(hip, fakenet.make_forward("pos", 99), 24)
    return hip.e, _dumps(hip.e)


def test_shapes_one_by_one_and_every_line(small):
    e, dumps = small
    _assert_equal(e.lines_host(1, 1), _model(dumps, None, 1, 1), "1 x 1")
    # more lines than any root has children, over outputs pre-filled with 0xAA bytes: every element is written
    G, n, m = 3, 128, 7
    fill = lambda dt: torch.full((G * n * m * dt.itemsize,), 0xAA, dtype=torch.uint8, device=e.dev).view(dt).reshape(G, n, m)
    mv, vs, q = fill(torch.int16), fill(torch.int32), fill(torch.float32)
    ln = torch.full((G * n * 2,), 0xAA, dtype=torch.uint8, device=e.dev).view(torch.int16).reshape(G, n)
    e.ctx.call("cz_search_lines", None, n, m, mv, vs, q, ln)
    got = dict(moves=mv.cpu().numpy().view(np.uint16), visits=vs.cpu().numpy(), q=q.cpu().numpy(), len=ln.cpu().numpy().view(np.uint16))
    _assert_equal(got, _model(dumps, None, n, m), "128 lines")
    counts = e.root_stats_host()["count"]
    for g in range(G):
        assert (got["len"][g, :counts[g]] >= 1).all() and not got["len"][g, counts[g]:].any()


def test_optional_outputs_may_be_null(small):
    e, dumps = small
    want = _model(dumps, None, 4, 6)
    for skip in ("moves", "visits", "q"):
        bufs = dict(moves=torch.empty((3, 4, 6), dtype=torch.int16, device=e.dev), visits=torch.empty((3, 4, 6), dtype=torch.int32, device=e.dev),
                    q=torch.empty((3, 4, 6), dtype=torch.float32, device=e.dev), len=torch.empty((3, 4), dtype=torch.int16, device=e.dev))
        e.ctx.call("cz_search_lines", None, 4, 6, *[None if k == skip else bufs[k] for k in ("moves", "visits", "q")], bufs["len"])
        got = dict(moves=bufs["moves"].cpu().numpy().view(np.uint16), visits=bufs["visits"].cpu().numpy(), q=bufs["q"].cpu().numpy(),
                   len=bufs["len"].cpu().numpy().view(np.uint16))
        for k in ("moves", "visits", "len"):
            assert k == skip or np.array_equal(got[k], want[k]), (skip, k)
        assert skip == "q" or np.array_equal(got["q"].view(np.uint32), want["q"].view(np.uint32)), skip


def test_bad_limits_raise_without_a_launch(small):
    from cchess_zero_amd._lib import CchessHipError
    e, _ = small
    for n_lines, max_len in ((0, 4), (129, 4), (4, 65), (4, 0), (-1, 4)):
        with pytest.raises(CchessHipError, match="cz_search_lines"):
            e.lines(n_lines, max_len)
    _assert_equal(e.lines_host(128, 64), _model(small[1], None, 128, 64), "the limits themselves")


def test_fresh_roots_have_no_lines(rules_golden):
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    hip = _Hip(5)
    hip.reset(boards[:5], side[:5], rr[:5])
    got = hip.e.lines_host(3, 4)
    assert not got["len"].any() and (got["moves"] == 0xFFFF).all() and not got["visits"].any() and not got["q"].view(np.uint32).any()
    mask = np.full((5, 66), -1, np.int32)
    assert not hip.e.lines_host(3, 4, allowed=mask)["len"].any()


def test_width_four_after_complete_steps(rules_golden):
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    hip = _Hip(8, width=4)
    hip.reset(boards[8:16], side[8:16], rr[8:16])
    fake = fakenet.make_forward("pos", 7)

    def forward(planes):
        logits, value = fake(planes.float().cpu().numpy())
        return torch.from_numpy(logits).cuda(), torch.from_numpy(value).cuda()
    hip.e.search(forward, 40)
    dumps = _dumps(hip.e)
    assert max(int(d[:, LM.N].max()) for d in dumps) > 1
    _assert_equal(hip.e.lines_host(6, 8), _model(dumps, None, 6, 8), "width 4")
