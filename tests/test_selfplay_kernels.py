"""k_sp_choose, k_sp_adjudicate and k_sp_flush (csrc/cz_selfplay.hip) against the float64 host model of
tests/selfplay_model.py, exactly.

  a  the golden self-play games, UNFORCED: the device loop is handed each game's own Dirichlet vectors and uniforms (the
     reference's numpy stream) and must play the reference's games move for move, records and z included;
  b  picks at the edges through the raw ABI: roots with 2-103 children (children 64-127 included), 0 / 1 / 7 / 200 playouts,
     temperatures 1, 0.5, 1e-3, noise eps 0, 0.25, 1 with gamma rows holding zeros and a dominant entry, u = 0, the
     largest float32 below 1, the midpoint of every child's CDF interval and random values;
  c  the records of K plies and the max_plies draw;
  d  min_sims gating and its pool-exhausted exemption, forced moves, BAD_ADVANCE and a root with no child;
  e  king captures and z over whole histories, the 60-ply tie, re-seeded and parked slots, adjudicate(played=...), the
     record ring's wrap-around and drop rule;
and the random inputs SelfPlay draws itself (Dirichlet(0.3) moments, u in [0, 1)).
Searches use the exact-integer fake net of tests/fakenet.py on the host.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fakenet
import selfplay_model as M

pytestmark = pytest.mark.gpu

START_FEN = "RNBAKABNR/9/1C5C1/P1P1P1P1P/9/9/p1p1p1p1p/1c5c1/9/rnbakabnr"
NONE = 0xFFFF
F32_TOP = float(np.nextafter(np.float32(1), np.float32(0)))   # the largest float32 below 1
_NO_NET = lambda planes: None   # step_ply's forward when the test has searched already (eng.search replaced)


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _lib():
    from cchess_zero_amd._lib import check, lib
    return lib(), check


def _engine(G, cap):
    from cchess_zero_amd.engine import SearchEngine
    return SearchEngine(G, cap, plane_dtype=torch.float32, channels=14)


def _search(eng, fwd, playouts, alive=None):
    """Root expansion, then playouts[g] simulations of tree g in lock-step; fwd(planes [n,9,10,14] f32, rows) -> (logits,
    value) is evaluated on the host for the rows that need the net only."""
    G = eng.G
    playouts = np.broadcast_to(np.asarray(playouts), (G,))
    alive = np.ones(G, bool) if alive is None else np.asarray(alive, bool)
    for i in range(-1, int(playouts.max(initial=0))):
        mask = alive if i < 0 else alive & (playouts > i)
        if not mask.any():
            break
        planes, need = eng.select(0 if i < 0 else 1, active=mask.astype(np.uint8))
        rows = np.nonzero(need.cpu().numpy())[0]
        lg = np.zeros((G, 2086), np.float32)
        v = np.zeros((G, 1), np.float32)
        if len(rows):
            lg[rows], v[rows] = fwd(planes[torch.from_numpy(rows).cuda()].cpu().numpy(), rows)
        eng.expand_backup(torch.from_numpy(lg).cuda(), torch.from_numpy(v).cuda())


def _one_net(salt=7):
    f = fakenet.make_forward("pos", salt)
    return lambda planes, rows: f(planes)


def _root(eng):
    st = eng.root_stats_host()
    k = st["count"].astype(np.int64)
    return st["label"], st["N"].astype(np.int64), k


def _begin(eng, max_plies, boards=None, side=None, rr=None):
    L, check = _lib()
    eng.ctx.bind_stream()
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda()
    bt, st, rt = dev(boards, np.uint8), dev(side, np.uint8), dev(rr, np.int32)
    check(L.cz_selfplay_begin(eng.ctx.h, int(max_plies), _vp(bt), _vp(st), _vp(rt)), "cz_selfplay_begin")
    torch.cuda.synchronize()


def _choose(eng, u, gamma=None, forced=None, temperature=1.0, eps=0.25, min_sims=0, out=None):
    """One k_sp_choose launch; u / gamma / forced host arrays or device tensors; -> played (host uint16 [G]) unless `out`."""
    L, check = _lib()
    G = eng.G
    dev = lambda a, dt: None if a is None else (a.contiguous() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dt)).cuda())
    ut, gt = dev(u, np.float32), dev(gamma, np.float32)
    assert out is None or out.is_contiguous()
    ft = None if forced is None else dev(np.asarray(forced, np.uint16).view(np.int16), np.int16)
    played = out if out is not None else torch.empty(G, dtype=torch.int16, device="cuda")
    eng.ctx.bind_stream()
    check(L.cz_selfplay_choose(eng.ctx.h, _vp(gt), _vp(ut), _vp(ft), float(temperature), float(eps), int(min_sims), _vp(played)),
          "cz_selfplay_choose")
    if out is None:
        return played.cpu().numpy().view(np.uint16).copy()


def _adjudicate(eng, reseed, played=None):
    L, check = _lib()
    fin = torch.full((eng.G,), -7, dtype=torch.int32, device="cuda")
    pt = None if played is None else torch.from_numpy(np.asarray(played, np.uint16).view(np.int16).copy()).cuda()
    eng.ctx.bind_stream()
    check(L.cz_selfplay_adjudicate(eng.ctx.h, int(reseed), _vp(pt), _vp(fin)), "cz_selfplay_adjudicate")
    return fin.cpu().numpy()


def _flush(eng, fin_n, offset, ring, read_cursor=None):
    L, check = _lib()
    fin = torch.from_numpy(np.asarray(fin_n, np.int32)).cuda()
    off = torch.from_numpy(np.asarray(offset, np.int64)).cuda()
    rc = None if read_cursor is None else torch.tensor([int(read_cursor)], dtype=torch.int64, device="cuda")
    eng.ctx.bind_stream()
    check(L.cz_selfplay_flush(eng.ctx.h, _vp(fin), _vp(off), _vp(ring), ring.shape[0], _vp(rc)), "cz_selfplay_flush")
    torch.cuda.synchronize()


def _stats(eng):
    from cchess_zero_amd._lib import SP_STATS
    L, check = _lib()
    s = torch.zeros(len(SP_STATS), dtype=torch.int64, device="cuda")
    eng.ctx.bind_stream()
    check(L.cz_selfplay_stats(eng.ctx.h, _vp(s)), "cz_selfplay_stats")
    return dict(zip(SP_STATS, (int(x) for x in s.cpu().numpy())))


def _records(boards, side, labels, visits, k, z, ply):
    """pack_records of one tree's root, rows beyond k padded like the kernel's (label 0xFFFF, visits 0)."""
    from cchess_zero_amd.selfplay import pack_records
    n = len(z)
    lab = np.full((n, 128), NONE, np.uint16)
    vis = np.zeros((n, 128), np.int64)
    lab[:, :k], vis[:, :k] = labels[:k], visits[:k]
    return pack_records(np.tile(boards, (n, 1)), np.full(n, side), lab, vis, np.full(n, k), z, ply=np.asarray(ply))


def _gamma_rows(rng, counts, zero_rows=()):
    """Gamma(0.3) rows with about a quarter of the children's entries zero and one dominant child; beyond a row's k junk that
    must never be read; rows in zero_rows sum to 0 over their children (no noise)."""
    G = len(counts)
    g = rng.gamma(0.3, size=(G, 128))
    for r in range(G):
        k = int(counts[r])
        g[r, :k][rng.random(k) < 0.25] = 0.0
        g[r, int(rng.integers(k))] = 50.0 * (1.0 + g[r, :k].sum())
        g[r, k:] = 1e4
        if r in zero_rows:
            g[r, :k] = 0.0
    return g.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# a. the golden games, unforced

def test_unforced_golden_replay_plays_the_reference_games():
    from cchess_zero_amd.selfplay import SelfPlay, canonical_boards, to_dense, unpack_records
    from oracle import oracle as O
    cases = M.golden_games()
    G = len(cases)
    playouts = np.array([c["meta"]["playout"] for c in cases])
    fwds = [fakenet.make_forward(c["meta"]["mode"], c["meta"]["salt"]) for c in cases]
    streams = [M.golden_stream(c["meta"]["seed"], c["count"]) for c in cases]

    def fwd(planes, rows):   # per-game fake nets (each golden game has its own salt)
        out = [fwds[g](planes[i:i + 1]) for i, g in enumerate(rows)]
        return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    eng = _engine(G, 60000)
    sp = SelfPlay(eng, None, int(playouts.max()), exploration=True, temperature=1.0, seed=1, max_plies=512, continuous=False)
    sp.start(np.tile(O.fen_to_board(START_FEN), (G, 1)), np.zeros(G, np.uint8),
             np.array([c["meta"].get("rr0", 0) for c in cases], np.int32))
    eng.search = lambda f, n, active=None: _search(eng, fwd, playouts, sp.active().numpy().astype(bool))
    n_plies = np.array([c["meta"]["plies"] for c in cases])
    gz = np.load(os.path.join(M.GOLDEN, "selfplay.npz"))
    for ply in range(int(n_plies.max())):
        gamma = np.full((G, 128), 3.0, np.float32)   # beyond a game's k children: anything
        u = np.full(G, 0.5, np.float32)
        for g, c in enumerate(cases):
            if ply < n_plies[g]:
                d, uu = streams[g][ply]
                gamma[g, :len(d)], u[g] = d, uu
        sp.step_ply(_NO_NET, rand=(gamma, u))
        played = sp.played.cpu().numpy().view(np.uint16)
        for g, c in enumerate(cases):
            want = c["played"][ply] if ply < n_plies[g] else NONE
            assert played[g] == want, (c["meta"]["name"], ply)
    rec = sp.drain()
    st = sp.stats()
    want = M.stats_ref([M.replay_golden(c)[1][-1] for c in cases])
    assert {k: st[k] for k in want} == want and st["dropped"] == 0
    assert st["sims"] == int((playouts * n_plies).sum())
    assert not bool(sp.active().any())
    u_ = unpack_records(rec)
    _, pi, z = to_dense(rec, 1.0, exact=True)
    starts = list(np.nonzero(u_["ply"] == 0)[0]) + [len(rec)]
    seen = set()
    for a, b in zip(starts[:-1], starts[1:]):
        match = [i for i, c in enumerate(cases) if n_plies[i] == b - a and i not in seen
                 and np.array_equal(u_["visits"][a:b].astype(np.int32), c["visits"])]
        assert match, "a finished game matches no golden game"
        c = cases[match[0]]
        seen.add(match[0])
        gp = np.zeros((b - a, 2086))
        for j, r in enumerate(np.nonzero(gz["case"] == match[0])[0]):
            lo, hi = int(gz["pi_ptr"][r]), int(gz["pi_ptr"][r + 1])
            gp[j, gz["pi_idx"][lo:hi]] = gz["pi_val"][lo:hi]
        assert np.array_equal(u_["ply"][a:b], np.arange(b - a))
        assert np.array_equal(u_["labels"][a:b], c["labels"]) and np.array_equal(u_["counts"][a:b], c["count"])
        assert np.array_equal(u_["side"][a:b], c["side"])
        assert np.array_equal(canonical_boards(u_["boards"][a:b], u_["side"][a:b]), c["state"])
        assert np.array_equal(pi[a:b], gp)                            # float64, bit for bit
        assert np.array_equal(z[a:b].astype(np.float64), c["z"])
    assert len(seen) == G


# ---------------------------------------------------------------------------------------------------------------------
# b / c. searched trees with 2-103 root children

@pytest.fixture(scope="module")
def trees():
    """50 roots (the start position, corpus positions of rules.npz, open boards with 65-103 moves) x playouts 0, 1, 7, 200:
    200 trees searched once with the fake net."""
    from conftest import open_boards
    from oracle import oracle as O
    g = np.load(os.path.join(M.GOLDEN, "rules.npz"))
    ok = [i for i in range(len(g["counts"])) if (g["boards"][i] == 1).any() and (g["boards"][i] == 8).any()]
    ok.sort(key=lambda i: (int(g["counts"][i]), i))
    corpus = [ok[int(j)] for j in np.linspace(0, len(ok) - 1, 21)]
    ob, os_ = open_boards(90, 5)
    n_ob = np.array([len(O.legal_moves(ob[i], int(os_[i]))) for i in range(len(ob))])
    wide = [i for i in np.argsort(n_ob, kind="stable") if 65 <= n_ob[i] <= 127]
    wide = [wide[int(j)] for j in np.linspace(0, len(wide) - 1, 28)]     # 28 of them, from 65 to 103 moves
    assert len(set(wide)) == 28
    roots = np.concatenate([O.fen_to_board(START_FEN)[None], g["boards"][corpus], ob[wide]])
    rside = np.concatenate([[0], g["side"][corpus], os_[wide]]).astype(np.uint8)
    R = len(roots)
    levels = np.array([0, 1, 7, 200])
    boards, side = np.repeat(roots, 4, axis=0), np.repeat(rside, 4)
    playouts = np.tile(levels, R)
    eng = _engine(len(boards), 24576)
    eng.reset(boards, side, None)
    _search(eng, _one_net(), playouts)
    labels, N, k = _root(eng)
    st, nodes, sims, _ = (x.cpu().numpy() for x in eng.status())
    assert (k >= 1).all() and k.max() >= 100 and (k > 64).sum() >= 4 * 28
    assert not st.any() and np.array_equal(sims, playouts)
    assert np.array_equal(N.sum(axis=1), playouts)
    return dict(eng=eng, boards=boards, side=side, playouts=playouts, labels=labels, N=N, k=k)


def test_choose_picks_exactly_at_the_edges(trees):
    eng, N, k, labels = trees["eng"], trees["N"], trees["k"], trees["labels"]
    G = eng.G
    rng = np.random.default_rng(2024)
    _begin(eng, 1)
    margins, hit, can_hit, draws = [], set(), set(), 0
    for temperature in (1.0, 0.5, 1e-3):
        for eps in (0.0, 0.25, 1.0):
            gamma = _gamma_rows(rng, k, zero_rows=set(range(5, G, 11)))
            cols = []
            for g in range(G):
                gm = gamma[g].astype(np.float64)
                p, lo, hi = M.intervals(N[g, :k[g]], temperature, gm, eps)
                us = [0.0, F32_TOP, 1.0] + list(rng.random(8).astype(np.float32).astype(np.float64))
                for i in np.nonzero(p > 0)[0]:
                    m = float(np.float32((lo[i] + hi[i]) / 2))
                    if lo[i] < m < hi[i] and min(m - lo[i], hi[i] - m) > 1e-9:
                        us.append(m)
                        can_hit.add((g, int(i)))
                cols.append(us)
            D = max(len(c) for c in cols)
            u = np.ascontiguousarray(np.array([c + list(rng.random(D - len(c)).astype(np.float32).astype(np.float64))
                                               for c in cols], np.float64).T)            # [D, G]: row d = draw d of every tree
            u_dev = torch.from_numpy(u.astype(np.float32)).cuda()
            g_dev = torch.from_numpy(gamma).cuda()
            out = torch.empty((D, G), dtype=torch.int16, device="cuda")
            for d in range(D):
                _choose(eng, u_dev[d], g_dev, None, temperature, eps, out=out[d])
            played = out.cpu().numpy().view(np.uint16)
            for g in range(G):
                kk = int(k[g])
                p = M.choice_probs(N[g, :kk], temperature, gamma[g].astype(np.float64), eps)
                i, margin = M.choose_ref(N[g, :kk], temperature, gamma[g].astype(np.float64), eps, u[:, g])
                bad = np.nonzero(played[:, g] != labels[g, i])[0]
                assert not len(bad), (temperature, eps, g, int(kk), int(trees["playouts"][g]), float(u[bad[0], g]),
                                      int(played[bad[0], g]), int(labels[g, i[bad[0]]]))
                assert (p[i] > 0).all()
                hit.update((g, int(j)) for j in i)
                margins.append(margin[np.isfinite(margin)])
                draws += D
    margins = np.concatenate(margins)
    print("k_sp_choose: %d draws, %d distinct (tree, child) picked, smallest margin %.3g" % (draws, len(hit), margins.min()))
    assert (margins < 1e-12).sum() == 0
    assert can_hit <= hit
    assert len({(g, i) for g, i in hit if i >= 64}) >= 200 and max(i for _, i in hit) == k.max() - 1


def test_records_of_k_plies_and_the_max_plies_draw(trees):
    eng, N, k, labels = trees["eng"], trees["N"], trees["k"], trees["labels"]
    G, K = eng.G, 3
    rng = np.random.default_rng(5)
    _begin(eng, K)
    for j in range(K):
        _choose(eng, rng.random(G), rng.gamma(0.3, size=(G, 128)), None, 1.0, 0.25)
    fin = _adjudicate(eng, 0, None)
    assert (fin == K).all()
    st = _stats(eng)
    assert st == dict(games=G, red_wins=0, black_wins=0, draws=G, plies=G * K, stalled=0, dropped=0,
                      sims=K * int(trees["playouts"].sum()))
    ring = torch.full((G * K + 5, 608), 0xA5, dtype=torch.uint8, device="cuda")
    _flush(eng, fin, np.arange(G) * K, ring, read_cursor=0)
    got = ring.cpu().numpy()
    for g in range(G):
        want = _records(trees["boards"][g], trees["side"][g], labels[g], N[g], int(k[g]), np.zeros(K), np.arange(K))
        assert np.array_equal(got[g * K:(g + 1) * K], want), g
    assert (got[G * K:] == 0xA5).all()
    # parked: nothing moves any more
    assert (_choose(eng, np.zeros(G)) == NONE).all() and (_adjudicate(eng, 0, None) == 0).all() and _stats(eng) == st


# ---------------------------------------------------------------------------------------------------------------------
# d. gating and overrides

def test_min_sims_gating_and_the_pool_exhausted_exemption():
    from oracle import oracle as O
    G = 6
    b = np.tile(O.fen_to_board(START_FEN), (G, 1))
    playouts = np.array([3, 7, 40, 3, 7, 40])
    eng = _engine(G, 1000)                      # ~45 nodes per simulation: the 40-playout trees fill their pools
    eng.reset(b, np.zeros(G, np.uint8), None)
    _search(eng, _one_net(), playouts)
    labels, N, k = _root(eng)
    status, _, sims, _ = (x.cpu().numpy() for x in eng.status())
    full = playouts == 40
    assert np.array_equal((status & 1) != 0, full) and np.array_equal(sims[~full], playouts[~full]) and (sims[full] < 40).all()
    _begin(eng, 2)
    u = np.array([0.1, 0.3, 0.5, 0.7, 0.9, 0.2])
    want = lambda g: labels[g, M.choose_ref(N[g, :k[g]], 1.0, None, 0.0, float(np.float32(u[g])))[0]]
    p1 = _choose(eng, u, None, None, 1.0, 0.0, min_sims=100)      # nobody has 100 simulations: only the full pools move
    assert all(p1[g] == (want(g) if full[g] else NONE) for g in range(G))
    p2 = _choose(eng, u, None, None, 1.0, 0.0, min_sims=7)        # 7 simulations are enough, 3 are not
    assert all(p2[g] == (NONE if playouts[g] == 3 else want(g)) for g in range(G))
    fin = _adjudicate(eng, 0, None)                               # max_plies 2: the full pools have moved twice
    assert np.array_equal(fin, np.where(full, 2, 0))
    p3 = _choose(eng, u, None, None, 1.0, 0.0, min_sims=0)
    assert all(p3[g] == (NONE if full[g] else want(g)) for g in range(G))
    fin2 = _adjudicate(eng, 0, None)
    assert np.array_equal(fin2, np.where(playouts == 7, 2, 0))    # no record and no ply for a gated tree
    assert _stats(eng)["sims"] == int(2 * sims[full].sum() + 2 * sims[playouts == 7].sum() + sims[playouts == 3].sum())
    fin_all = fin + fin2
    ring = torch.zeros((16, 608), dtype=torch.uint8, device="cuda")
    _flush(eng, fin_all, np.concatenate([[0], np.cumsum(fin_all)[:-1]]), ring)
    got, r = ring.cpu().numpy(), 0
    for g in range(G):
        if fin_all[g]:
            want_rec = _records(b[g], 0, labels[g], N[g], int(k[g]), np.zeros(2), np.arange(2))
            assert np.array_equal(got[r:r + 2], want_rec), g
            r += 2


def test_forced_moves_bad_advance_and_a_root_without_children():
    from conftest import open_boards
    from oracle import oracle as O
    ob, os_ = open_boards(30, 9)
    n_ob = np.array([len(O.legal_moves(ob[i], int(os_[i]))) for i in range(len(ob))])
    i = int(np.argmax(n_ob))
    assert n_ob[i] > 72
    G = 4
    boards, side = np.tile(ob[i], (G, 1)), np.full(G, os_[i], np.uint8)
    eng = _engine(G, 8192)
    eng.reset(boards, side, None)
    _search(eng, _one_net(), 3)
    labels, N, k = _root(eng)
    moves = O.legal_moves(ob[i], int(os_[i]))
    keeps = [j for j in range(len(moves)) if O.apply_move(ob[i], int(moves[j]))[2] == 0]   # moves that take no king
    hi = [j for j in keeps if j >= 64][-1]
    lo_ = keeps[0]
    own = set(int(m) for m in moves)
    other = [int(m) for m in O.legal_moves(ob[i], 1 - int(os_[i])) if int(m) not in own][0]   # not a root child
    forced = np.array([labels[0, hi], labels[1, lo_], NONE, other], np.uint16)
    _begin(eng, 1)
    u = np.full(G, 0.37)
    played = _choose(eng, u, None, forced, 1.0, 0.0)
    sampled = labels[2, M.choose_ref(N[2, :k[2]], 1.0, None, 0.0, float(np.float32(0.37)))[0]]
    assert np.array_equal(played, [labels[0, hi], labels[1, lo_], sampled, other])
    eng.advance(played)
    b_after, s_after, _ = (x.cpu().numpy() for x in eng.root_state())
    status = eng.status()[0].cpu().numpy()
    for g in range(3):
        assert np.array_equal(b_after[g], O.apply_move(ob[i], int(played[g]))[0]) and s_after[g] == 1 - os_[i]
    assert not (status[:3] & 8).any() and status[3] & 8
    # max_plies 1: every game that moved ends with its record (a draw unless the move took a king); the bad advance stalls
    outs = []
    for g in range(3):
        nb, cap, _ = O.apply_move(ob[i], int(played[g]))
        outs.append(M.adjudicate_ref(nb, 0 if cap else 1, 1, [os_[i]], 1))
    outs.append(M.adjudicate_ref(ob[i], 1, 1, [os_[i]], 1, stalled=True))
    fin = _adjudicate(eng, 1, None)
    assert np.array_equal(fin, [o.fin_n for o in outs]) and np.array_equal(fin, [1, 1, 1, 0])
    st = _stats(eng)
    assert {k_: st[k_] for k_ in M.stats_ref(outs)} == M.stats_ref(outs) and st["sims"] == 12 and st["dropped"] == 0
    ring = torch.zeros((3, 608), dtype=torch.uint8, device="cuda")
    _flush(eng, fin, [0, 1, 2, 3], ring)
    got = ring.cpu().numpy()
    for g in range(3):
        assert np.array_equal(got[g], _records(ob[i], os_[i], labels[g], N[g], int(k[g]), outs[g].z, [0])[0]), g
    # re-seeded: the start position again, a fresh root, the BAD_ADVANCE flag gone
    b2, s2, _ = (x.cpu().numpy() for x in eng.root_state())
    st, nodes, sims, _ = (x.cpu().numpy() for x in eng.status())
    assert (b2 == ob[i]).all() and (s2 == os_[i]).all() and not st.any() and (nodes == 1).all() and not sims.any()

    # a root with no child: a 2-node pool cannot hold the root's expansion
    eng2 = _engine(2, 2)
    eng2.reset(np.tile(O.fen_to_board(START_FEN), (2, 1)), np.zeros(2, np.uint8), None)
    _search(eng2, _one_net(), 0)
    _begin(eng2, 4)
    assert (_choose(eng2, [0.5, 0.5], None, [NONE, 44], 1.0, 0.0) == NONE).all()
    assert (_adjudicate(eng2, 0, None) == 0).all()
    assert _stats(eng2) == dict(games=2, red_wins=0, black_wins=0, draws=0, plies=0, stalled=2, dropped=0, sims=0)


# ---------------------------------------------------------------------------------------------------------------------
# e. adjudication and the ring

def _king_capture(board, side):
    """The first legal move of `side` that takes the other king, or None."""
    from oracle import oracle as O
    for m in O.legal_moves(board, side):
        nb = O.apply_move(board, int(m))[0]
        if not ((nb == M.KING_RED).any() and (nb == M.KING_BLACK).any()):
            return int(m)
    return None


def test_king_captures_give_z_over_the_whole_history():
    """Kings facing on an open file and a rook each: a few sampled plies, then the mover takes the king as soon as it can.
    Every ply's pick, fin_n, the records with their z and the win counters against the model."""
    from cchess_zero_amd.selfplay import SelfPlay
    from oracle import oracle as O
    fens = ["4K4/9/9/9/R8/8r/9/9/9/4k4", "3K5/9/9/3R5/9/9/5r3/9/9/3k5", "4K4/4A4/9/2R6/9/9/6r2/9/4a4/4k4",
            "5K3/9/9/9/1R7/7r1/9/9/9/5k3"]
    boards = np.stack([O.fen_to_board(f) for f in fens for _ in (0, 1)])
    side = np.array([0, 1] * 4, np.uint8)
    G = len(boards)
    S = 1 + np.arange(G) % 3                                     # sampled plies before the capture is forced
    eng = _engine(G, 8192)
    sp = SelfPlay(eng, None, 6, exploration=True, temperature=1.0, seed=1, max_plies=64, continuous=False)
    sp.start(boards, side, np.zeros(G, np.int32))
    net = _one_net(31)
    rng = np.random.default_rng(77)
    board, sd, rr = boards.copy(), side.astype(np.int64), np.zeros(G, np.int64)
    hist = [[] for _ in range(G)]
    alive = np.ones(G, bool)
    outcomes, want_ring = [None] * G, []
    for ply in range(30):
        if not alive.any():
            break
        _search(eng, net, 6, alive)
        labels, N, k = _root(eng)
        gamma = rng.gamma(0.3, size=(G, 128)).astype(np.float32)
        u = rng.random(G).astype(np.float32)
        forced = np.full(G, NONE, np.uint16)
        want = np.full(G, NONE, np.uint16)
        for g in np.nonzero(alive)[0]:
            cap = _king_capture(board[g], int(sd[g])) if ply >= S[g] else None
            if cap is not None:
                forced[g] = want[g] = cap
            else:
                want[g] = labels[g, M.choose_ref(N[g, :k[g]], 1.0, gamma[g].astype(np.float64), 0.25, float(u[g]))[0]]
            hist[g].append((board[g].copy(), int(sd[g]), labels[g].copy(), N[g].copy(), int(k[g])))
        eng.search = lambda f, n, active=None: None              # searched above
        sp.step_ply(_NO_NET, forced=forced, rand=(gamma, u))
        played = sp.played.cpu().numpy().view(np.uint16)
        assert np.array_equal(played, want), ply
        fin = sp.fin_n.cpu().numpy()
        assert not fin[~alive].any()
        for g in np.nonzero(alive)[0]:
            nb, cap, _ = O.apply_move(board[g], int(want[g]))
            board[g], sd[g], rr[g] = nb, 1 - sd[g], 0 if cap else rr[g] + 1
            out = M.adjudicate_ref(nb, rr[g], len(hist[g]), [h[1] for h in hist[g]], 64)
            assert fin[g] == (out.fin_n if out else 0), (ply, g)
            if out:
                alive[g] = False
                outcomes[g] = out
                for j, (b0, s0, lab, vis, kk) in enumerate(hist[g]):
                    want_ring.append(_records(b0, s0, lab, vis, kk, out.z[j:j + 1], [j]))
    rec = sp.drain()
    done = [o for o in outcomes if o is not None]
    print("king captures:", outcomes)
    assert np.array_equal(rec, np.concatenate(want_ring))
    st = sp.stats()
    assert {k_: st[k_] for k_ in M.stats_ref(done)} == M.stats_ref(done)
    assert st["red_wins"] >= 1 and st["black_wins"] >= 1 and st["red_wins"] + st["black_wins"] >= G - 1


def test_sixty_ply_tie_reseed_and_parked_slots():
    from oracle import oracle as O
    start = O.fen_to_board(START_FEN)
    moves = O.legal_moves(start, 0)
    caps = [int(m) for m in moves if O.apply_move(start, int(m))[1]]
    quiet = int(next(m for m in moves if not O.apply_move(start, int(m))[1]))
    assert caps
    G = 4
    eng = _engine(G, 4096)
    eng.reset(np.tile(start, (G, 1)), np.zeros(G, np.uint8), np.array([59, 59, 58, 59], np.int32))
    _search(eng, _one_net(), [2, 2, 2, 1])
    labels, N, k = _root(eng)
    _begin(eng, 512)
    forced = np.array([quiet, caps[0], quiet, NONE], np.uint16)
    played = _choose(eng, np.full(G, 0.5), None, forced, 1.0, 0.0, min_sims=2)   # slot 3 waits (1 < 2 simulations)
    assert np.array_equal(played, [quiet, caps[0], quiet, NONE])
    eng.advance(played)
    fin = _adjudicate(eng, 1, played)
    assert np.array_equal(fin, [1, 0, 0, 0])                  # rr 60: the tie; a capture resets rr; rr 59 goes on
    b, s, rr = (x.cpu().numpy() for x in eng.root_state())
    st, nodes, sims, _ = (x.cpu().numpy() for x in eng.status())
    # re-seeded: the start board, side and restrict_round of the slot, a fresh root
    assert np.array_equal(b[0], start) and s[0] == 0 and rr[0] == 59 and st[0] == 0 and nodes[0] == 1 and sims[0] == 0
    assert np.array_equal(rr[1:], [0, 59, 59]) and np.array_equal(s, [0, 1, 1, 0]) and sims[3] == 1
    st_ = _stats(eng)
    assert st_["draws"] == 1 and st_["games"] == 1 and st_["plies"] == 1 and st_["sims"] == 6
    ring = torch.zeros((2, 608), dtype=torch.uint8, device="cuda")
    _flush(eng, fin, [0, 1, 1, 1], ring)
    assert np.array_equal(ring.cpu().numpy()[0], _records(start, 0, labels[0], N[0], int(k[0]), [0], [0])[0])
    # the re-seeded slot plays its next game from ply 0: the same tie again, recorded as ply 0
    _search(eng, _one_net(), 2, [1, 0, 0, 0])
    labels, N, k = _root(eng)
    played = _choose(eng, np.full(G, 0.5), None, [quiet, NONE, NONE, NONE], 1.0, 0.0, min_sims=2)
    assert np.array_equal(played, [quiet, NONE, NONE, NONE])
    eng.advance(played)
    fin = _adjudicate(eng, 0, played)
    assert np.array_equal(fin, [1, 0, 0, 0])
    _flush(eng, fin, [1, 2, 2, 2], ring)
    assert np.array_equal(ring.cpu().numpy()[1], _records(start, 0, labels[0], N[0], int(k[0]), [0], [0])[0])

    # adjudicate(played=...) skips a slot that did not move even when its position is over; parked slots stay parked
    nok = start.copy()
    nok[nok == M.KING_BLACK] = 0
    eng2 = _engine(2, 256)
    eng2.reset(np.stack([nok, start]), np.zeros(2, np.uint8), None)
    _begin(eng2, 8)
    assert np.array_equal(_adjudicate(eng2, 0, [NONE, NONE]), [0, 0]) and _stats(eng2)["games"] == 0
    assert np.array_equal(_adjudicate(eng2, 0, None), [0, 0])
    st2 = _stats(eng2)
    assert st2["games"] == 1 and st2["red_wins"] == 1 and st2["plies"] == 0
    _search(eng2, _one_net(), 1, [0, 1])
    before = [x.cpu().numpy().copy() for x in eng2.root_state()]
    assert _choose(eng2, [0.5, 0.5], None, None, 1.0, 0.0)[0] == NONE
    assert np.array_equal(_adjudicate(eng2, 1, None), [0, 0])
    after = [x.cpu().numpy() for x in eng2.root_state()]
    assert all(np.array_equal(x[0], y[0]) for x, y in zip(before, after))
    st3 = _stats(eng2)
    assert st3["games"] == 1 and st3["sims"] == 1


def test_record_ring_wraps_and_drops_whole_games():
    from oracle import oracle as O
    G, K, R = 8, 8, 37
    start = O.fen_to_board(START_FEN)
    eng = _engine(G, 4096)
    eng.reset(np.tile(start, (G, 1)), np.zeros(G, np.uint8), None)
    _search(eng, _one_net(), 2)
    labels, N, k = _root(eng)
    _begin(eng, K)
    for j in range(K):
        _choose(eng, np.full(G, (j + 0.5) / K), None, None, 1.0, 0.0)
    hist = [_records(start, 0, labels[g], N[g], int(k[g]), np.zeros(K), np.arange(K)) for g in range(G)]
    sentinel = np.full((R, 608), 0x5C, np.uint8)

    def run(fin_n, cursor, read_cursor):
        offset = cursor + np.concatenate([[0], np.cumsum(fin_n)[:-1]])
        ring = torch.from_numpy(sentinel.copy()).cuda()
        before = _stats(eng)["dropped"]
        _flush(eng, fin_n, offset, ring, read_cursor)
        want, dropped = M.flush_ref(sentinel, hist, fin_n, offset, read_cursor)
        assert np.array_equal(ring.cpu().numpy(), want)
        assert _stats(eng)["dropped"] - before == dropped
        return want, dropped

    # no read cursor: offsets 30 .. 59 wrap past row 36
    fin_n = np.array([5, 0, 8, 3, 7, 2, 4, 1])
    want, dropped = run(fin_n, 30, None)
    assert dropped == 0 and (want[23:30] == 0x5C).all()
    # read cursor 18: rows up to 55 may be written — the game of 2 ends there exactly and is written, the next (6) is dropped
    # whole, its rows (18 .. 23, undrained) keep their bytes
    fin_n = np.array([5, 0, 8, 3, 7, 2, 6, 0])
    want, dropped = run(fin_n, 30, 18)
    assert dropped == 6 and (want[18:30] == 0x5C).all() and np.array_equal(want[17], hist[5][1])
    # one row less of room: the game of 2 goes too
    want, dropped = run(fin_n, 30, 17)
    assert dropped == 8 and np.array_equal(want[15], hist[4][6]) and (want[16:30] == 0x5C).all()


# ---------------------------------------------------------------------------------------------------------------------
# the random inputs SelfPlay draws itself

def test_random_inputs_are_dirichlet_0_3_and_uniforms():
    """Normalised over a game's first k entries, SelfPlay.random_inputs' gamma rows are Dirichlet(0.3): mean 1/k per
    component and variance (1/k)(1-1/k)/(0.3k+1).  8192 rows; the variance is held to 4 % (k >= 44) and 5 % (k = 2),
    over 6 standard errors of the estimate (0.35 % / 0.7 % at this size; alpha 0.25 or 0.35 moves it by 14-19 % at k = 44).
    The raw variates are Gamma(0.3, 1): mean 0.3 within 6 standard errors.  u lies in [0, 1)."""
    from cchess_zero_amd.selfplay import SelfPlay
    from oracle import oracle as O
    G = 1024
    eng = _engine(G, 64)
    sp = SelfPlay(eng, None, 1, exploration=True, seed=123, max_plies=1)
    sp.start(np.tile(O.fen_to_board(START_FEN), (G, 1)), np.zeros(G, np.uint8))
    draws = [sp.random_inputs() for _ in range(8)]
    gam = torch.cat([d[0] for d in draws]).double().cpu().numpy()
    u = torch.cat([d[1] for d in draws]).cpu().numpy()
    assert gam.shape == (8 * G, 128) and u.dtype == np.float32
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) < 6 * np.sqrt(1 / 12 / len(u))
    assert abs(gam.mean() - 0.3) < 6 * np.sqrt(0.3 / gam.size)
    for kk, tol in ((2, 0.05), (44, 0.04), (100, 0.04)):
        x = gam[:, :kk] / gam[:, :kk].sum(axis=1, keepdims=True)
        var = (1.0 / kk) * (1 - 1.0 / kk) / (0.3 * kk + 1)
        assert np.abs(x.mean(axis=0) - 1.0 / kk).max() < 6 * np.sqrt(var / len(x)), kk
        assert abs(x.var() / var - 1) < tol, (kk, x.var() / var)
    sp.exploration = False
    g2, u2 = sp.random_inputs()
    assert g2 is None and u2.shape == (G,)
