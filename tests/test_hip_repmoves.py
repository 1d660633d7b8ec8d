"""cz_repetition_moves (k_repetition_moves around cz_repmoves.h's wave_repetition_moves) on the GPU, bit for bit against
tests/repmoves_model.py and against the composed path of public calls — king-safe list -> successors -> king-safe lists of the
children -> successors -> hash / flags / threats of every child and grandchild -> extended records -> repetition(_chase): the
constructed cases and the random walks of the CPU test, batch sizes around the wave, record lengths up to 129 and len == stride,
windows and chase records given or NULL, folds 2, 3 and 8, a losing candidate behind index 63, mated / kingless / refused boards,
and the raw C ABI at odd addresses with every output NULL in turn."""
import ctypes as C

import numpy as np
import pytest
import torch

import repmoves_model as M

pytestmark = pytest.mark.gpu
NAMES = ("moves", "count", "verdict", "reply", "reply_verdict", "allowed", "summary")


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


def pack(cases, stride=None, chase=True, window=True):
    """cases -> the arrays of one call (the records padded to `stride` with zeros); window False: NULL, every case must mean
    "all earlier positions" then"""
    G = len(cases)
    stride = stride or max(len(c["keys"]) for c in cases)
    keys, checks, recs = np.zeros((G, stride), np.uint64), np.zeros((G, stride), np.uint8), np.zeros((G, stride, 4), np.uint64)
    length, win = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for g, c in enumerate(cases):
        n = len(c["keys"])
        keys[g, :n], checks[g, :n], length[g] = c["keys"], c["checks"], n
        if chase:
            recs[g, :n] = np.array(c["recs"], np.uint64).reshape(n, 4)
        assert window or c["window"] is None or c["window"] >= n - 1
        win[g] = n - 1 if c["window"] is None else c["window"]
    return dict(boards=np.stack([c["board"] for c in cases]), side=np.array([c["side"] for c in cases], np.uint8), keys=keys.view(np.int64),
                in_check=checks, chase=recs.view(np.int64) if chase else None, length=length, window=win if window else None)


def host(out):
    return dict(moves=out["moves"].cpu().numpy().view(np.uint16), count=out["count"].cpu().numpy().view(np.uint16), verdict=out["verdict"].cpu().numpy(),
                reply=out["reply"].cpu().numpy().view(np.uint16), reply_verdict=out["reply_verdict"].cpu().numpy(),
                allowed=out["allowed"].cpu().numpy().view(np.uint32), summary=out["summary"].cpu().numpy())


def model_rows(cases):
    rows = [M.rows(M.model_of(c)) for c in cases]
    return {k: np.stack([np.asarray(r[i]) for r in rows]) for i, k in enumerate(NAMES)}


def same(got, want, what):
    for k in NAMES:
        bad = np.nonzero((np.asarray(got[k]).reshape(len(want[k]), -1) != np.asarray(want[k]).reshape(len(want[k]), -1)).any(axis=1))[0]
        assert len(bad) == 0, (what, k, bad[:5], np.asarray(got[k])[bad[:2]], np.asarray(want[k])[bad[:2]])


def fused(rules, a, fold):
    return host(rules.repetition_moves(a["boards"], a["side"], a["keys"], a["in_check"], a["chase"], a["length"], a["window"], fold))


def composed(rules, a, fold):
    """The same answer from the public calls, one launch each per level; the reduction over replies and moves in NumPy"""
    dev = rules.dev
    t = lambda x, d: None if x is None else torch.as_tensor(x, dtype=d, device=dev)
    boards, side = t(a["boards"], torch.uint8), t(a["side"], torch.uint8)
    keys, chk, rec = t(a["keys"], torch.int64), t(a["in_check"], torch.uint8), t(a["chase"], torch.int64)
    G, stride = keys.shape
    length = t(a["length"], torch.int64)
    valid = (length >= 1) & (length <= stride)
    win = (length - 1 if a["window"] is None else torch.minimum(t(a["window"], torch.int64).clamp(min=0), length - 1))
    mv, cnt, mask, _ = rules.movegen_kingsafe(boards, side)

    def level(b, s, m, c, par_keys, par_chk, par_rec, par_len, par_win):
        """The children of a level: their boards and lists, their records (the parent's with the child behind it), windows and
        verdicts"""
        cb, cs, cap, par, lab = rules.successors(b, s, m, c)
        par = par.to(torch.int64)
        T = cb.shape[0]
        k = torch.cat([par_keys[par], torch.zeros((T, 1), dtype=torch.int64, device=dev)], 1)
        f = torch.cat([par_chk[par], torch.zeros((T, 1), dtype=torch.uint8, device=dev)], 1)
        ln = par_len[par]
        at = ln.clamp(0, k.shape[1] - 1).unsqueeze(1)
        k.scatter_(1, at, rules.hash(cb, cs).unsqueeze(1))
        f.scatter_(1, at, (rules.in_check(cb, cs) & 1).unsqueeze(1))
        r = None
        if par_rec is not None:
            r = torch.cat([par_rec[par], torch.zeros((T, 1, 4), dtype=torch.int64, device=dev)], 1)
            r.scatter_(1, at.unsqueeze(2).expand(T, 1, 4), rules.threats(cb, cs).unsqueeze(1))
        w = torch.where(cap != 0, torch.zeros_like(ln), torch.minimum(par_win[par] + 1, ln))
        L = (ln + 1).to(torch.int32)
        if r is not None:
            v, _, cause = rules.repetition_chase(k, f, r, cs, L, w.to(torch.int32), fold)
        else:
            v, _ = rules.repetition(k, f, cs, L, w.to(torch.int32), fold)
            cause = ((v == M.RED_LOSES) | (v == M.BLACK_LOSES)).to(torch.uint8)
        code = torch.where(valid_of(par), v | (cause << 4), torch.zeros_like(v))
        return cb, cs, par, lab, k, f, r, ln + 1, w, code

    valid_of = lambda par: valid[par]
    cb, cs, par1, lab1, k1, f1, r1, l1, w1, own = level(boards, side, mv, cnt, keys, chk, rec, length, win)
    cmv, ccnt, _, _ = rules.movegen_kingsafe(cb, cs)
    valid_of = lambda par: valid[par1[par]]
    _, _, par2, lab2, _, _, _, _, _, rep = level(cb, cs, cmv, ccnt, k1, f1, r1, l1, w1)
    cnt_h, own_h, par1_h = cnt.cpu().numpy().astype(np.int64), own.cpu().numpy(), par1.cpu().numpy()
    rep_h, par2_h, lab2_h = rep.cpu().numpy(), par2.cpu().numpy(), lab2.cpu().numpy().view(np.uint16)
    side_h, mv_h = np.asarray(a["side"]), mv.cpu().numpy().view(np.uint16)
    T = len(own_h)
    reply, rv = np.full(T, 0xFFFF, np.uint16), np.zeros(T, np.uint8)
    loss_of_child = np.where(side_h[par1_h] != 0, M.BLACK_LOSES, M.RED_LOSES)
    for i in np.nonzero((rep_h & 15) == loss_of_child[par2_h])[0][::-1]:          # the first one in order wins
        reply[par2_h[i]], rv[par2_h[i]] = lab2_h[i], rep_h[i]
    out = dict(moves=mv_h, count=cnt.cpu().numpy().view(np.uint16), verdict=np.zeros((G, 128), np.uint8), reply=np.full((G, 128), 0xFFFF, np.uint16),
               reply_verdict=np.zeros((G, 128), np.uint8), allowed=mask.cpu().numpy().view(np.uint32).copy(), summary=np.zeros(G, np.uint8))
    off = np.concatenate([[0], np.cumsum(np.maximum(cnt_h, 0))])
    for g in range(G):
        n = int(cnt_h[g])
        if n < 0:
            for k in ("moves", "verdict", "reply", "reply_verdict", "allowed"):
                out[k][g] = 0
            continue
        sl = slice(off[g], off[g] + n)
        out["verdict"][g, :n], out["reply"][g, :n], out["reply_verdict"][g, :n] = own_h[sl], reply[sl], rv[sl]
        lm, lo = (M.BLACK_LOSES, M.RED_LOSES) if side_h[g] else (M.RED_LOSES, M.BLACK_LOSES)
        losing = ((own_h[sl] & 15) == lm) | (((own_h[sl] & 15) == M.NONE) & (rv[sl] != 0))
        forced = n > 0 and losing.all()
        removed = losing.any() and not forced
        if removed:
            for l in mv_h[g, :n][losing]:
                out["allowed"][g, int(l) >> 5] &= ~np.uint32(1 << (int(l) & 31))
        out["summary"][g] = (M.REMOVED if removed else 0) | (M.FORCED if forced else 0) | (M.OPP_LOSES if ((own_h[sl] & 15) == lo).any() else 0)
    return out


def by_call(cases):
    """The cases grouped into calls: one per (fold, chase records or not)"""
    groups = {}
    for c in cases:
        groups.setdefault((c["fold"], c["recs"] is not None), []).append(c)
    return groups


def test_constructed_cases_against_the_model_and_the_composed_path(rules):
    for (fold, chase), cases in by_call(M.constructed_cases()).items():
        a = pack(cases, chase=chase)
        got = fused(rules, a, fold)
        same(got, model_rows(cases), ("model", fold, chase))
        same(got, composed(rules, a, fold), ("composed", fold, chase))
    j = M.wide_case()[1]
    wide = [c for c in M.constructed_cases() if c["name"] == "wide"][0]
    got = fused(rules, pack([wide], chase=False), 2)
    assert j >= 64 and got["count"][0] > 64 and got["verdict"][0, j] & 15 in (M.RED_LOSES, M.BLACK_LOSES) and got["summary"][0] & M.REMOVED
    assert not (got["allowed"][0, got["moves"][0, j] >> 5] >> (got["moves"][0, j] & 31)) & 1


@pytest.mark.parametrize("G", [1, 63, 64, 65])
def test_random_walks_batch_sizes(rules, G):
    ref = M.walk_reference()
    step = max(1, len(ref) // G)
    cases = [ref[(i * step) % len(ref)] for i in range(G)]
    a = pack(cases)
    got = fused(rules, a, M.WALK_FOLD)
    same(got, model_rows(cases), ("model", G))
    same(got, composed(rules, a, M.WALK_FOLD), ("composed", G))


def test_random_walks_whole_corpus_chase_null_and_window_null(rules):
    ref = M.walk_reference()
    a = pack(ref)
    got = fused(rules, a, M.WALK_FOLD)
    same(got, model_rows(ref), "model")
    found = sum(int((r & 15 != 0).sum()) for r in got["verdict"]) + int((got["reply_verdict"] != 0).sum())
    assert found >= len(ref) // 10, found
    for fold in (2, 3):               # without the chase records and without windows: the composed path alone
        b = dict(a, chase=None, window=None)
        same(fused(rules, b, fold), composed(rules, b, fold), ("composed, NULL chase and window", fold))


def long_cases():
    """The perpetual line with made-up plies in the middle: record lengths 1, 2, 63, 64, 65 and 129, the repeated positions more
    than 64 plies apart; folds 2, 3, 8; windows given (short, long) or all; with and without chase records"""
    import chase_cases as CC
    import repetition_cases as RC
    boards, sides, _ = CC.play_line(RC.perpetual_board(), 0, RC.PERPETUAL_LINE * 7)
    keys, checks, recs = M.history_of(boards, sides)
    out = []
    for L in (1, 2, 63, 64, 65, 129):
        for fold in (2, 3, 8):
            real = L if L <= 2 else (27 if L % 2 else 28)         # the real positions: 3 at the start, the others at the end
            pad = L - real
            k = keys[:3] + [90000 + i for i in range(pad)] + keys[3:real]
            c = checks[:3] + [i & 1 for i in range(pad)] + checks[3:real]
            r = recs[:3] + [[0, 0, 0, 0]] * pad + recs[3:real]
            k, c, r = k[:L], c[:L], r[:L]
            for window in (None, 5, 70):
                for chase in (True, False):
                    out.append(M.case("long %d fold %d window %s" % (L, fold, window), boards[real - 1], sides[real - 1], k, c, r if chase else None, window, fold))
    return out


def test_record_lengths_windows_folds(rules):
    flagged = 0
    for (fold, chase), cases in by_call(long_cases()).items():
        want = model_rows(cases)
        flagged += int((want["summary"] != 0).sum())
        same(fused(rules, pack(cases, stride=140, chase=chase), fold), want, ("stride 140", fold, chase))
        for L in sorted(set(len(c["keys"]) for c in cases)):                      # len == stride, window NULL
            sub = [c for c in cases if len(c["keys"]) == L and c["window"] is None]
            a = pack(sub, stride=L, chase=chase, window=False)
            got = fused(rules, a, fold)
            same(got, model_rows(sub), ("len == stride", L, fold, chase))
            same(got, composed(rules, a, fold), ("composed, len == stride", L, fold, chase))
    assert flagged >= 12


def test_mated_kingless_refused_and_bad_lengths(rules):
    import chase_cases as CC
    mated = CC.board(["Rd5", "Re1"], kings=("Kf0", "kd9"))
    kingless = CC.board(["Ra4", "cb7"], kings=("ke9",))
    refused = np.zeros(90, np.uint8)
    refused[:3], refused[84] = 3, 8
    cases = [M.case("mated", mated, 1, [1, 2, 3], [0, 0, 1], None, None, 3), M.case("kingless", kingless, 0, [1, 2], [0, 0], None, None, 3),
             M.case("refused", refused, 0, [5], [0], None, None, 3), M.case("fine", CC.CHASE_BOARD, 0, [7], [0], None, None, 3)]
    a = pack(cases, stride=4, chase=False)
    got = fused(rules, a, 3)
    want = model_rows([cases[0], cases[1], cases[3]])
    same({k: got[k][[0, 1, 3]] for k in NAMES}, want, "model")
    assert got["count"][0] == 0 and got["summary"][0] == 0 and not got["allowed"][0].any() and got["count"][1] > 0
    assert got["count"][2] == 0xFFFF and all(not got[k][2].any() for k in NAMES if k != "count")
    same(got, composed(rules, a, 3), "composed")
    # a length outside 1 .. stride: the list and the whole set, no verdict, nothing read
    walk = [c for c in M.walk_reference() if c["res"]["summary"]][:4]
    a = pack(walk)
    base = fused(rules, a, M.WALK_FOLD)
    for bad in (0, -3, a["keys"].shape[1] + 1):
        b = dict(a, length=np.full(len(walk), bad, np.int32))
        got = fused(rules, b, M.WALK_FOLD)
        assert np.array_equal(got["moves"], base["moves"]) and np.array_equal(got["count"], base["count"])
        assert not got["verdict"].any() and not got["reply_verdict"].any() and not got["summary"].any() and (got["reply"] == 0xFFFF).all()
        mv, cnt, mask, _ = rules.movegen_kingsafe(a["boards"], a["side"])
        assert np.array_equal(got["allowed"], mask.cpu().numpy().view(np.uint32))


def test_raw_abi_odd_addresses_null_outputs_and_refusals(rules):
    from cchess_zero_amd._lib import lib
    L, h = lib(), rules.ctx.h
    ref = M.walk_reference()
    cases = [c for c in ref if c["res"]["summary"]][:5]
    G = len(cases)
    a = pack(cases)
    want = model_rows(cases)
    stride = a["keys"].shape[1]
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())

    def buf(nbytes, o, fill=0x5A):
        t = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
        assert t.data_ptr() % 16 == 0
        return t[o:o + nbytes]

    def put(arr, o):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        b = buf(len(raw), o)
        b.copy_(torch.from_numpy(raw.copy()).cuda())
        return b
    rules.ctx.bind_stream()
    # inputs and outputs at the oddest address their element type allows; one row of sentinel behind every output
    inp = [put(a["boards"], 1), put(a["side"], 3), put(a["keys"], 8), put(a["in_check"], 5), put(a["chase"], 8), put(a["length"], 4), put(a["window"], 4)]
    size = dict(moves=256, count=2, verdict=128, reply=256, reply_verdict=128, allowed=264, summary=1)
    odd = dict(moves=16, count=2, verdict=1, reply=2, reply_verdict=3, allowed=4, summary=7)
    dt = dict(moves=np.uint16, count=np.uint16, verdict=np.uint8, reply=np.uint16, reply_verdict=np.uint8, allowed=np.uint32, summary=np.uint8)

    def run(skip=None, shift=None):
        outs = {k: buf((G + 1) * size[k], odd[k] if shift is None else shift.get(k, odd[k])) for k in NAMES}
        rc = L.cz_repetition_moves(h, p(inp[0]), p(inp[1]), p(inp[2]), p(inp[3]), p(inp[4]), stride, p(inp[5]), p(inp[6]), G, M.WALK_FOLD,
                                   *[None if k == skip else p(outs[k]) for k in NAMES])
        torch.cuda.synchronize()
        return rc, {k: outs[k].cpu().numpy().copy().view(dt[k]).reshape(G + 1, -1) for k in NAMES}
    rc, got = run()
    assert rc == 0
    same({k: got[k][:G] for k in NAMES}, want, "odd addresses")
    assert all((got[k][G:].view(np.uint8) == 0x5A).all() for k in NAMES)
    for skip in NAMES:                                        # every output NULL in turn: the others are the same
        rc, got = run(skip=skip)
        assert rc == 0 and (got[skip].view(np.uint8) == 0x5A).all()
        for k in NAMES:
            if k != skip:
                assert np.array_equal(got[k][:G].reshape(np.asarray(want[k]).shape), want[k]), (skip, k)
    rc, got = run(shift=dict(moves=8))
    assert rc == -1 and all((got[k].view(np.uint8) == 0x5A).all() for k in NAMES)                      # moves not 16-byte aligned
    args = [p(x) for x in inp]
    outs = [p(buf((G + 1) * size[k], odd[k])) for k in NAMES]
    call = lambda ctx, i, G_, fold, o: L.cz_repetition_moves(ctx, i[0], i[1], i[2], i[3], i[4], stride, i[5], i[6], G_, fold, *o)
    assert call(h, args, 0, 2, outs) == 0 and call(h, [None] * 7, 0, 2, [None] * 7) == 0               # G = 0: nothing happens
    assert call(None, args, G, 2, outs) == -1 and call(h, args, -1, 2, outs) == -1
    assert call(h, args, G, 1, outs) == -1 and call(h, args, G, 9, outs) == -1 and call(h, args, G, 2, [None] * 7) == -1
    for i in (0, 1, 2, 3, 5):                                                                         # chase and window may be NULL
        assert call(h, args[:i] + [None] + args[i + 1:], G, 2, outs) == -1
    assert L.cz_repetition_moves(h, *args[:5], 0, args[5], args[6], G, 2, *outs) == -1                # stride 0
