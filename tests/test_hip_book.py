"""The opening book on the GPU (csrc/cz_book.hip; cchess_zero_amd.book) against tests/book_model.py, exactly: cz_book_keys,
cz_book_entries, Book.build, cz_book_probe and cz_book_choose on a corpus of replayed games — 256 random games under each rule
level, the file-mirrored copy of every fourth, three hand-written lines — then the argument checks of the C ABI, Book.playout and
arena.book_openings, the Analyzer's book= and the command line."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import book_model as BM
from oracle import oracle as O

pytestmark = pytest.mark.gpu
SEED, SEED2 = 11, 12
HAND = [["h2e2", "h9g7", "h0g2", "i9h9"], ["b2e2", "b9c7", "b0c2"], ["c3c4", "h9g7", "b0c2"]]
U64 = 2 ** 64 - 1


@pytest.fixture(scope="module")
def bk():
    from cchess_zero_amd.book import Book
    return Book()


def _mirrored_games(games):
    m = BM.mirror_table()
    return [g._replace(labels=tuple(int(m[l]) for l in g.labels)) for g in games]


def _replay(bk, games, rules):
    from cchess_zero_amd.games import GameReplayer
    r = GameReplayer(ctx=bk.ctx).replay(games, rules=rules, on_illegal="drop")
    assert r.counts["kept_games"] == len(games) and r.counts["kept_plies"] == sum(len(g.labels) for g in games)
    return r.records


@pytest.fixture(scope="module")
def corpus(bk):
    from cchess_zero_amd import games as GA
    from cchess_zero_amd._lib import tables
    rng = np.random.default_rng(SEED)
    lists = {}
    for i, rules in enumerate(("xiangqi", "capture")):
        rg = GA.random_games(rules, 256, SEED + i, 40, device=bk.ctx.device.index)
        gs = GA.games_from_labels(rg["moves"], rg["lens"], rng.integers(-1, 2, 256))
        lists[rules] = gs + _mirrored_games(gs[::4])
    l2i = tables()["label2i"]
    b0, s0, rr0 = GA._start()
    lists["xiangqi"] += [GA.Game(b0, s0, rr0, tuple(l2i[m] for m in line), int(r), ()) for line, r in zip(HAND, (1, 0, -1))]
    rec_x, rec_c = _replay(bk, lists["xiangqi"], "xiangqi"), _replay(bk, lists["capture"], "capture")
    dev = torch.cat([rec_x, rec_c]).contiguous()
    rec = dev.cpu().numpy()
    key, label, outcome = BM.entries(rec, 40)
    mkey, mir = BM.keys(rec[:, :90], rec[:, 90])
    assert np.array_equal(key, mkey) and (outcome != 255).all()
    book = BM.reduce(key, label, outcome)
    # what the corpus has to hold (the seed is chosen so that it does)
    assert (mir == 0).sum() >= 100 and (mir == 1).sum() >= 100 and (mir == 2).sum() >= 3
    assert np.unique(book[0], return_counts=True)[1].max() >= 3 and int(book[2].max()) >= 3
    return dict(games=lists, dev=dev, rec=rec, nx=len(rec_x), boards=np.ascontiguousarray(rec[:, :90]), side=np.ascontiguousarray(rec[:, 90]),
                key=key, mir=mir, entries=(key, label, outcome), book=book)


@pytest.fixture(scope="module")
def built(bk, corpus):
    from cchess_zero_amd.book import Book
    return Book(bk.ctx).build(corpus["dev"], 40)


def raw(bk, name, *args):
    """lib().<name>(ctx, ...) as it is: the return code, no exception"""
    from cchess_zero_amd._lib import lib
    bk.ctx.bind_stream()
    rc = getattr(lib(), name)(bk.ctx.h, *[C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args])
    torch.cuda.synchronize()
    return rc


def dev(a, dt):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u" and a.dtype.itemsize > 1:
        a = a.view("i%d" % a.dtype.itemsize)
    return torch.as_tensor(a).cuda().to(dt).contiguous()


def u(t, dt):
    return t.cpu().numpy().view(dt)


# ---- cz_book_keys ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 63, 64, 65, 129, 0])
def test_keys(bk, corpus, G):
    G = G or len(corpus["rec"])
    hb, hs = corpus["boards"][-G:], corpus["side"][-G:]
    side = dev(hs, torch.uint8)
    for off in (0, 2):                                  # 16-byte aligned boards, and the byte path
        buf = torch.zeros(G * 90 + 16, dtype=torch.uint8, device="cuda")
        buf[off:off + G * 90] = torch.from_numpy(hb.reshape(-1)).cuda()
        boards = buf[off:off + G * 90]
        assert boards.data_ptr() % 16 == off
        key = torch.full((G + 2,), 0x1234, dtype=torch.int64, device="cuda")
        mir = torch.full((G + 2,), 77, dtype=torch.uint8, device="cuda")
        assert raw(bk, "cz_book_keys", boards, side, G, key, mir) == 0
        assert np.array_equal(u(key, np.uint64)[:G], corpus["key"][-G:]) and np.array_equal(u(mir, np.uint8)[:G], corpus["mir"][-G:])
        assert (u(key, np.uint64)[G:] == 0x1234).all() and (u(mir, np.uint8)[G:] == 77).all()
        key2 = torch.full((G + 2,), 0x1234, dtype=torch.int64, device="cuda")
        assert raw(bk, "cz_book_keys", boards, side, G, key2, None) == 0            # mirrored = NULL
        assert torch.equal(key, key2)


def test_keys_a_byte_above_14_is_an_empty_square(bk, corpus):
    hb, hs = corpus["boards"][:70].copy(), corpus["side"][:70]
    for i in range(70):
        hb[i, (7 * i) % 90] = 200 if i % 2 else 15
    want_key, want_mir = BM.keys(hb, hs)
    cleared = np.where(hb > 14, 0, hb).astype(np.uint8)
    assert np.array_equal(want_key, BM.keys(cleared, hs)[0]) and not np.array_equal(want_key, corpus["key"][:70])
    key = torch.empty(70, dtype=torch.int64, device="cuda")
    mir = torch.empty(70, dtype=torch.uint8, device="cuda")
    assert raw(bk, "cz_book_keys", dev(hb, torch.uint8), dev(hs, torch.uint8), 70, key, mir) == 0
    assert np.array_equal(u(key, np.uint64), want_key) and np.array_equal(u(mir, np.uint8), want_mir)


# ---- cz_book_entries ------------------------------------------------------------------------------------------------------------
def _entries(bk, rec, max_ply):
    n = len(rec)
    key = torch.full((n + 1,), 0x1234, dtype=torch.int64, device="cuda")
    label = torch.full((n + 1,), 0x55, dtype=torch.int16, device="cuda")
    outcome = torch.full((n + 1,), 0x55, dtype=torch.uint8, device="cuda")
    assert raw(bk, "cz_book_entries", rec, n, max_ply, key, label, outcome) == 0
    assert int(key[n]) == 0x1234 and int(label[n]) == 0x55 and int(outcome[n]) == 0x55
    return u(key, np.uint64)[:n], u(label, np.uint16)[:n], u(outcome, np.uint8)[:n]


@pytest.mark.parametrize("max_ply", [0, 1, 7, 40])
def test_entries(bk, corpus, max_ply):
    rec = corpus["rec"]
    want = BM.entries(rec, max_ply)
    ply = rec[:, 94].astype(np.int64) | rec[:, 95].astype(np.int64) << 8
    assert np.array_equal(want[2] == 255, (ply >= max_ply) if max_ply else np.zeros(len(rec), bool))
    assert 0 < (want[2] == 255).sum() < len(rec) or max_ply in (0, 40)
    for n in (1, 63, 65, len(rec)):
        got = _entries(bk, corpus["dev"][len(rec) - n:], max_ply)
        for g, w in zip(got, want):
            assert np.array_equal(g, w[len(rec) - n:]), (n, max_ply)


def test_entries_count_zero_and_tied_visits(bk, corpus):
    rec = corpus["rec"][:130].copy()
    rec[3, 91] = 0                                                           # no child: no entry
    rec[64, 91] = 0
    for i in (5, 66, 129):                                                   # every visit equal: the first child
        rec[i, 352:608] = np.full(128, 9, np.uint16).view(np.uint8)
    at = int(rec[7, 352:608].view(np.uint16).argmax())                       # two maxima: the first
    assert rec[7, 91] > at + 1 or at > 0
    other = at - 1 if at > 0 else at + 1
    v = rec[7, 352:608].view(np.uint16).copy()
    v[other] = v[at]
    rec[7, 352:608] = v.view(np.uint8)
    rec[9, 352:354] = np.array([65535], np.uint16).view(np.uint8)            # the largest count is no negative number
    want = BM.entries(rec, 40)
    assert want[2][3] == 255 and want[2][64] == 255 and want[1][3] == 0xFFFF
    got = _entries(bk, dev(rec, torch.uint8), 40)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    first = rec[:, 96:98].copy().view(np.uint16)[:, 0]
    for i in (5, 9, 66, 129):
        assert got[1][i] == BM.canonical_label(int(first[i]), int(corpus["mir"][i]))


# ---- Book.build -----------------------------------------------------------------------------------------------------------------
def test_build_equals_the_model(bk, corpus, built):
    for g, w in zip(built.arrays(), corpus["book"]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert built.source_plies == len(corpus["rec"]) and built.max_ply == 40
    from cchess_zero_amd.book import Book
    host = Book(bk.ctx).build(corpus["rec"][:500], 7)                         # a host array, another bound
    for g, w in zip(host.arrays(), BM.book_of(corpus["rec"][:500], 7)):
        assert np.array_equal(g, w)


def test_build_of_the_mirrored_corpus_is_the_same_book(bk, corpus, built):
    from cchess_zero_amd.book import Book
    rec = torch.cat([_replay(bk, _mirrored_games(corpus["games"][r]), r) for r in ("xiangqi", "capture")])
    assert not torch.equal(rec, corpus["dev"])
    other = Book(bk.ctx).build(rec, 40)
    for g, w in zip(other.arrays(), built.arrays()):
        assert g.tobytes() == w.tobytes()


# ---- cz_book_probe --------------------------------------------------------------------------------------------------------------
def _probe(bk, bkey, boards, side):
    G = len(side)
    first = torch.full((G + 1,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((G + 1,), -7, dtype=torch.int32, device="cuda")
    mir = torch.full((G + 1,), 77, dtype=torch.uint8, device="cuda")
    assert raw(bk, "cz_book_probe", len(bkey), dev(bkey, torch.int64) if len(bkey) else None, dev(boards, torch.uint8), dev(side, torch.uint8), G, first, count,
               mir) == 0
    assert int(first[G]) == -7 and int(count[G]) == -7 and int(mir[G]) == 77
    return u(first, np.int32)[:G], u(count, np.int32)[:G], u(mir, np.uint8)[:G]


def _hold(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_probe_every_corpus_position_hits(bk, corpus):
    got = _probe(bk, corpus["book"][0], corpus["boards"], corpus["side"])
    _hold(got, BM.probe(corpus["book"][0], corpus["boards"], corpus["side"]))
    assert (got[0] >= 0).all() and (got[1] >= 1).all() and got[1].max() >= 3


def test_probe_positions_outside_the_book_miss(bk, corpus):
    from cchess_zero_amd import games as GA
    rg = GA.random_games("xiangqi", 256, SEED2, 40, device=bk.ctx.device.index)
    deep = rg["lens"] >= 30
    boards, side = rg["final_boards"][deep], rg["final_side"][deep]
    assert len(side) >= 30
    got = _probe(bk, corpus["book"][0], boards, side)
    _hold(got, BM.probe(corpus["book"][0], boards, side))
    assert (got[0] == -1).mean() >= 0.9 and ((got[0] == -1) == (got[1] == 0)).all()


def test_probe_small_books_and_the_ends(bk, corpus):
    bkey = corpus["book"][0]
    ends = np.concatenate([np.nonzero(corpus["key"] == bkey[0])[0][:2], np.nonzero(corpus["key"] == bkey[-1])[0][:2]])
    assert len(ends) >= 2
    idx = np.concatenate([ends, np.arange(0, len(corpus["key"]), 41)])
    boards, side = corpus["boards"][idx], corpus["side"][idx]
    for E in (0, 1, 2, len(bkey)):
        got = _probe(bk, bkey[:E], boards, side)
        _hold(got, BM.probe(bkey[:E], boards, side))
        if E == 0:
            assert (got[0] == -1).all() and (got[1] == 0).all()
    full = _probe(bk, bkey, boards, side)
    assert full[0][0] == 0 and full[0][len(ends) - 1] + full[1][len(ends) - 1] == len(bkey)
    mid = len(bkey) // 2
    one = bkey[mid:mid + 1]
    got = _probe(bk, one, boards, side)
    _hold(got, BM.probe(one, boards, side))
    k = corpus["key"][idx]
    assert (k < one[0]).any() and (k > one[0]).any() and (got[0][k != one[0]] == -1).all()


# ---- cz_book_choose -------------------------------------------------------------------------------------------------------------
def _choose(bk, book, boards, side, allowed, min_games, mode, rnd):
    G = len(side)
    played = torch.full((G + 1,), 0x55, dtype=torch.int16, device="cuda")
    index = torch.full((G + 1,), -7, dtype=torch.int32, device="cuda")
    args = (len(book[0]), dev(book[0], torch.int64), dev(book[1], torch.int16), dev(book[2], torch.int32), boards, side, allowed, G, min_games, mode,
            None if rnd is None else dev(rnd, torch.int32))
    assert raw(bk, "cz_book_choose", *args, played, index) == 0
    assert int(played[G]) == 0x55 and int(index[G]) == -7
    played2 = torch.empty(G, dtype=torch.int16, device="cuda")
    assert raw(bk, "cz_book_choose", *args, played2, None) == 0 and torch.equal(played2, played[:G])     # index = NULL
    return u(played, np.uint16)[:G], u(index, np.int32)[:G]


@pytest.fixture(scope="module")
def probed(corpus):
    return BM.probe(corpus["book"][0], corpus["boards"], corpus["side"])


@pytest.fixture(scope="module")
def rnd(corpus):
    r = np.random.default_rng(SEED).integers(0, 2 ** 32, len(corpus["side"]), dtype=np.uint64).astype(np.uint32)
    r[::5], r[1::5] = 0, 0xFFFFFFFF
    return r


@pytest.mark.parametrize("min_games", [1, 2, 1000])
def test_choose_equals_the_model(bk, corpus, probed, rnd, min_games):
    boards, side = dev(corpus["boards"], torch.uint8), dev(corpus["side"], torch.uint8)
    picks = []
    for mode in (0, 1):
        got = _choose(bk, corpus["book"], boards, side, None, min_games, mode, rnd if mode else None)
        _hold(got, BM.choose(corpus["book"], None, None, None, min_games, mode, rnd, probed))
        assert ((got[0] == 0xFFFF) == (got[1] == -1)).all()
        assert (got[0] == 0xFFFF).all() if min_games == 1000 else (got[0] != 0xFFFF).any()
        picks.append(got[0])
    if min_games == 1:
        assert (picks[0] != 0xFFFF).all() and (picks[0] != picks[1]).any()


def test_choose_among_the_allowed_moves(bk, corpus, probed, rnd):
    from cchess_zero_amd.rules import Rules
    nx, book = corpus["nx"], corpus["book"]
    hb, hs = corpus["boards"][:nx], corpus["side"][:nx]
    boards, side = dev(hb, torch.uint8), dev(hs, torch.uint8)
    mask = Rules(ctx=bk.ctx).movegen_kingsafe(boards, side, want_moves=False)[2]
    hm = u(mask, np.uint32).copy()
    pr = tuple(x[:nx] for x in probed)
    first = {}
    for mode in (0, 1):
        got = _choose(bk, book, boards, side, mask, 1, mode, rnd[:nx])
        _hold(got, BM.choose(book, None, None, hm, 1, mode, rnd[:nx], pr))
        p = got[0].astype(np.int64)
        assert (p != 0xFFFF).all() and ((hm[np.arange(nx), p >> 5] >> (p & 31).astype(np.uint32)) & 1).all()     # every move of the corpus was king-safe
        first[mode] = got
    # the move chosen in mode 0 banned: never picked again, in either mode
    p0 = first[0][0].astype(np.int64)
    hm2 = hm.copy()
    hm2[np.arange(nx), p0 >> 5] &= ~(np.uint32(1) << (p0 & 31).astype(np.uint32))
    for mode in (0, 1):
        got = _choose(bk, book, boards, side, dev(hm2, torch.int32), 1, mode, rnd[:nx])
        _hold(got, BM.choose(book, None, None, hm2, 1, mode, rnd[:nx], pr))
        assert (got[0] != p0).all() and (got[0] == 0xFFFF).any() and (got[0] != 0xFFFF).any()
    # a mirrored position plays the mirror image of the stored label, a move of ITS board
    m, (played, index) = BM.mirror_table(), first[0]
    mirrored = np.nonzero(pr[2] == 1)[0][:200]
    assert len(mirrored) >= 100
    for g in mirrored:
        assert int(played[g]) == int(m[int(book[1][index[g]])]) and int(played[g]) in O.legal_moves(hb[g], int(hs[g])).tolist()


# ---- the C ABI's argument checks ------------------------------------------------------------------------------------------------
def test_argument_errors(bk, corpus):
    from cchess_zero_amd._lib import lib
    G = 8
    boards, side = dev(corpus["boards"][:G], torch.uint8), dev(corpus["side"][:G], torch.uint8)
    rec = corpus["dev"][:G]
    i64, i32, i16, u8 = (torch.zeros(G + 1, dtype=t, device="cuda") for t in (torch.int64, torch.int32, torch.int16, torch.uint8))
    bkey, blabel, bgames = (dev(a[:4], t) for a, t in zip(corpus["book"], (torch.int64, torch.int16, torch.int32)))
    odd = lambda t, by: C.c_void_p(t.data_ptr() + by)

    def bad(text, name, *args):
        from cchess_zero_amd._lib import lib
        bk.ctx.bind_stream()
        rc = getattr(lib(), name)(*[C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args])
        assert rc == -1 and text in lib().cz_last_error().decode(), (name, text, rc, lib().cz_last_error())
    h = bk.ctx.h
    bad("cz_book_keys: null ctx / negative G", "cz_book_keys", None, boards, side, G, i64, u8)
    bad("cz_book_keys: null ctx / negative G", "cz_book_keys", h, boards, side, -1, i64, u8)
    bad("cz_book_keys: boards, side, key required", "cz_book_keys", h, None, side, G, i64, u8)
    bad("cz_book_keys: boards, side, key required", "cz_book_keys", h, boards, side, G, None, u8)
    bad("cz_book_keys: key must be 8-byte aligned", "cz_book_keys", h, boards, side, G, odd(i64, 4), u8)
    bad("cz_book_entries: null ctx / negative n", "cz_book_entries", h, rec, -1, 40, i64, i16, u8)
    bad("cz_book_entries: max_ply >= 0", "cz_book_entries", h, rec, G, -1, i64, i16, u8)
    bad("cz_book_entries: records, key, label, outcome required", "cz_book_entries", h, rec, G, 40, i64, i16, None)
    bad("cz_book_entries: records must be 16-byte aligned", "cz_book_entries", h, odd(rec, 8), G - 1, 40, i64, i16, u8)
    bad("cz_book_entries: key must be 8-byte, label 2-byte aligned", "cz_book_entries", h, rec, G, 40, i64, odd(i16, 1), u8)
    bad("cz_book_probe: negative E", "cz_book_probe", h, -1, bkey, boards, side, G, i32, i32, u8)
    bad("cz_book_probe: boards, side, first, count, mirrored required", "cz_book_probe", h, 4, bkey, boards, side, G, i32, i32, None)
    bad("cz_book_probe: bkey required (E > 0)", "cz_book_probe", h, 4, None, boards, side, G, i32, i32, u8)
    bad("cz_book_probe: bkey must be 8-byte, first and count 4-byte aligned", "cz_book_probe", h, 3, odd(bkey, 4), boards, side, G, i32, i32, u8)
    bad("cz_book_probe: bkey must be 8-byte, first and count 4-byte aligned", "cz_book_probe", h, 4, bkey, boards, side, G, odd(i32, 2), i32, u8)
    ch = lambda **k: [k.get(n, v) for n, v in (("h", h), ("E", 4), ("bkey", bkey), ("blabel", blabel), ("bgames", bgames), ("boards", boards), ("side", side),
                                               ("allowed", None), ("G", G), ("min_games", 1), ("mode", 0), ("rnd", None), ("played", i16), ("index", i32))]
    bad("cz_book_choose: null ctx / negative G", "cz_book_choose", *ch(G=-1))
    bad("cz_book_choose: negative E", "cz_book_choose", *ch(E=-1))
    bad("cz_book_choose: mode is 0 (most games) or 1 (sample)", "cz_book_choose", *ch(mode=2))
    bad("cz_book_choose: negative min_games", "cz_book_choose", *ch(min_games=-1))
    bad("cz_book_choose: boards, side, played required", "cz_book_choose", *ch(played=None))
    bad("cz_book_choose: bkey, blabel, bgames required (E > 0)", "cz_book_choose", *ch(bgames=None))
    bad("cz_book_choose: rnd required in mode 1", "cz_book_choose", *ch(mode=1))
    bad("cz_book_choose: bkey must be 8-byte", "cz_book_choose", *ch(mode=1, rnd=odd(i32, 2)))
    bad("cz_book_choose: bkey must be 8-byte", "cz_book_choose", *ch(played=odd(i16, 1)))
    # G == 0 / n == 0: CZ_OK without a launch, whatever the arrays are
    assert lib().cz_book_keys(h, None, None, 0, None, None) == 0 and lib().cz_book_entries(h, None, 0, 40, None, None, None) == 0
    assert lib().cz_book_probe(h, 0, None, None, None, 0, None, None, None) == 0
    assert lib().cz_book_choose(h, 0, None, None, None, None, None, None, 0, 1, 1, None, None, None) == 0
    torch.cuda.synchronize()


# ---- Book.probe, playout, arena.book_openings -------------------------------------------------------------------------------------
def _walk(line, games_of, min_games):
    """the line from the opening position by the oracle, every (position, move) a book entry of at least min_games -> the position"""
    b, s = O.fen_to_board(O.START_FEN), 0
    for l in line:
        key, mir = BM.canonical(b, s)
        assert games_of.get((key, BM.canonical_label(l, mir)), 0) >= min_games, (line, l)
        assert l in O.legal_moves(b, s).tolist()
        b, _, _ = O.apply_move(b, l)
        s ^= 1
    return b, s


def test_probe_lists(built, corpus):
    idx = np.concatenate([np.nonzero(corpus["mir"] == v)[0][:3] for v in (0, 1, 2)])
    rows = built.probe(corpus["boards"][idx], corpus["side"][idx])
    first, count, mir = BM.probe(corpus["book"][0], corpus["boards"][idx], corpus["side"][idx])
    key, label, games, wins, draws = corpus["book"]
    for g in range(len(idx)):
        want = [dict(label=BM.own_label(int(label[i]), int(mir[g])), games=int(games[i]), wins=int(wins[i]), draws=int(draws[i]),
                     losses=int(games[i]) - int(wins[i]) - int(draws[i]), score=(int(wins[i]) + int(draws[i]) / 2.0) / int(games[i]))
                for i in range(first[g], first[g] + count[g])]
        assert rows[g] == sorted(want, key=lambda r: (-r["games"], r["label"])) and len(rows[g]) >= 1
    assert built.probe(np.zeros((1, 90), np.uint8), [0]) == [[]]


def test_playout_and_book_openings(built, corpus):
    from cchess_zero_amd import arena
    key, label, games = corpus["book"][:3]
    games_of = {(int(k), int(l)): int(g) for k, l, g in zip(key, label, games)}
    po = built.playout(64, 8, SEED)
    assert po.boards.shape == (64, 90) and (po.lens >= 1).all() and (po.lens == 8).any()
    for g in range(64):
        assert len(po.labels[g]) == po.lens[g]
        b, s = _walk(po.labels[g], games_of, 1)
        assert np.array_equal(b, po.boards[g]) and s == po.side[g] and (b == 1).sum() == 1 and (b == 8).sum() == 1
    again = built.playout(64, 8, SEED)
    assert np.array_equal(again.boards, po.boards) and again.labels == po.labels and np.array_equal(again.rr, po.rr)
    assert built.playout(64, 8, SEED + 1).labels != po.labels
    op = arena.book_openings(built, 16, 6, SEED)
    assert len(op) == 16 and len(set(op.keys.tolist())) == 16
    for i in range(16):
        assert len(op.moves[i]) == 6
        b, s = _walk(op.moves[i], games_of, 2)
        assert np.array_equal(b, op.boards[i]) and s == op.side[i] and (b == 1).sum() == 1 and (b == 8).sum() == 1
        assert int(op.keys[i]) == O.zhash(b, s) & U64
    again = arena.book_openings(built, 16, 6, SEED)
    assert np.array_equal(again.boards, op.boards) and again.moves == op.moves and np.array_equal(again.keys, op.keys)
    with pytest.raises(ValueError, match="only [0-9]+ distinct positions"):
        arena.book_openings(built, 2000, 6, SEED)


def test_analysis_with_a_book(built, corpus, tmp_path):
    from cchess_zero_amd.analysis import Analyzer
    from cchess_zero_amd.book import Book
    from cchess_zero_amd.net import PolicyValueNet
    an = Analyzer(PolicyValueNet(res_block_nums=1, seed=3), 16, 8)
    built.save(str(tmp_path / "b.npz"))
    book = Book(an.engine.ctx).load(str(tmp_path / "b.npz"))
    idx = np.nonzero(corpus["mir"][:corpus["nx"]] != 2)[0][:6].tolist() + [0, int(np.nonzero(corpus["mir"] == 1)[0][0])]
    pos = [(corpus["boards"][i], int(corpus["side"][i]), 0) for i in idx]
    plain = an.analyse(pos, n_lines=2, max_len=6)
    withbook = an.analyse(pos, n_lines=2, max_len=6, book=book)
    rows = book.probe(corpus["boards"][idx], corpus["side"][idx])
    for a, b, r in zip(plain, withbook, rows):
        assert "book" not in a and b["book"] == r and len(r) >= 1
        assert {k: v for k, v in b.items() if k != "book"} == a
    # the UCCI engine's searcher on the same context: the most played king-safe move with its counters, and never a banned one
    from cchess_zero_amd.ucci import AnalyzerSearcher
    s = AnalyzerSearcher(an)
    key, label, games, wins, draws = corpus["book"]
    for i in idx[:2] + idx[-2:]:
        b, sd = corpus["boards"][i], int(corpus["side"][i])
        s.set_position(b, sd, 0)
        mask, _ = s.kingsafe_mask()
        played, index = BM.choose(corpus["book"], b[None], [sd], mask[None], 1, 0, None)
        got = s.book(str(tmp_path / "b.npz"), mask, 1, False)
        j = int(index[0])
        assert j >= 0 and got == (int(played[0]), dict(games=int(games[j]), wins=int(wins[j]), draws=int(draws[j]), losses=int(games[j]) - int(wins[j]) - int(draws[j]),
                                                       score=(int(wins[j]) + int(draws[j]) / 2.0) / int(games[j])))
        assert s.book(str(tmp_path / "b.npz"), mask, 1000, False) is None
        ban = mask.copy()
        ban[got[0] >> 5] &= ~(np.uint32(1) << np.uint32(got[0] & 31))
        other = s.book(str(tmp_path / "b.npz"), ban, 1, True)
        assert other is None or (other[0] != got[0] and (int(mask[other[0] >> 5]) >> (other[0] & 31)) & 1)


def test_command_line_build_and_probe(bk, corpus, tmp_path, capsys):
    from cchess_zero_amd import book, games as GA
    gs = corpus["games"]["xiangqi"]
    pgn, out = str(tmp_path / "g.pgn"), str(tmp_path / "book.npz")
    open(pgn, "w").write(GA.write_games(gs, pgn=True))
    assert book.main(["--build", "--in", pgn, "--rules", "xiangqi", "--out", out]) == 0
    said = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = BM.book_of(corpus["rec"][:corpus["nx"]], 40)
    assert said == dict(games=len(gs), plies=corpus["nx"], entries=len(want[0]), positions=len(set(want[0].tolist())), skipped=0)
    from cchess_zero_amd.notation import START_FEN
    assert book.main(["--probe", "--book", out, "--fen", START_FEN]) == 0
    row = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    k0 = BM.canonical(O.fen_to_board(O.START_FEN), 0)[0]
    at = np.nonzero(want[0] == np.uint64(k0))[0]
    L = O.labels()
    model = sorted([(-int(want[2][i]), int(want[1][i]), int(want[3][i]), int(want[4][i])) for i in at])
    assert [(-m["games"], m["label"], m["wins"], m["draws"]) for m in row["moves"]] == model and len(model) >= 3
    assert [m["move"] for m in row["moves"]] == [L[l] for _, l, _, _ in model] and row["fen"] == START_FEN
    # --merge adds the same games once more
    assert book.main(["--build", "--in", pgn, "--rules", "xiangqi", "--merge", out, "--out", str(tmp_path / "twice.npz")]) == 0
    twice = book.Book(bk.ctx).load(str(tmp_path / "twice.npz"))
    assert np.array_equal(twice.key, want[0]) and np.array_equal(twice.games, 2 * want[2]) and twice.source_games == 2 * len(gs)
