"""tests/book_model.py against hand-written cases (no GPU): the canonical key and label under the left-right mirror, the reduce,
and the integer arithmetic of the sampled choice.  (The mirror table comes from libcchess_hip.so, which the build leaves in the
tree.)"""
import numpy as np
import pytest

import book_model as BM
from oracle import oracle as O

LINE = ["h2e2", "h9g7", "h0g2", "i9h9", "i0h0", "b9c7"]


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__
    __graft_entry__.build_hip_only()


def _start():
    return O.fen_to_board(O.START_FEN)


def test_the_start_position_is_self_mirror():
    key, mir = BM.canonical(_start(), 0)
    assert mir == 2 and key == O.zhash(_start(), 0) & (2 ** 64 - 1)
    assert BM.canonical(_start(), 1)[1] == 2 and BM.canonical(_start(), 1)[0] != key


def test_a_game_and_its_mirrored_twin_give_the_same_book():
    twin = BM.mirror_moves(LINE)
    assert twin[:2] == ["b2e2", "b9c7"] and twin != LINE
    a = BM.book_of(BM.records_of_game(LINE, 1), 40)
    b = BM.book_of(BM.records_of_game(twin, 1), 40)
    assert len(a[0]) == len(LINE)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert (np.diff(a[0].astype(object)) > 0).all()           # six positions, ascending keys


def test_h2e2_and_b2e2_are_one_entry_of_two_games():
    rec = np.concatenate([BM.records_of_game(["h2e2"], 1), BM.records_of_game(["b2e2"], -1)])
    key, label, games, wins, draws = BM.book_of(rec, 40)
    L = O.labels()
    assert len(key) == 1 and int(games[0]) == 2 and int(wins[0]) == 1 and int(draws[0]) == 0
    assert int(label[0]) == min(L.index("h2e2"), L.index("b2e2")) and int(key[0]) == BM.canonical(_start(), 0)[0]


def test_a_position_and_its_mirror_share_a_key_and_differ_in_mirrored():
    b, _, _ = O.apply_move(_start(), O.labels().index("h2e2"))
    m = BM.mirror_board(b)
    assert not np.array_equal(b, m)
    (k0, f0), (k1, f1) = BM.canonical(b, 1), BM.canonical(m, 1)
    assert k0 == k1 and {f0, f1} == {0, 1}
    # the same reply, written in either orientation, is one canonical label
    L, reply = O.labels(), "h9g7"
    assert BM.canonical_label(L.index(reply), f0) == BM.canonical_label(L.index(BM.mirror_moves([reply])[0]), f1)


def test_skipped_records_and_the_first_maximum():
    rec = BM.records_of_game(LINE, 0)
    key, label, outcome = BM.entries(rec, 3)
    assert outcome.tolist() == [1, 1, 1, 255, 255, 255] and label[3:].tolist() == [0xFFFF] * 3 and int(key[4]) == BM.canonical(rec[4, :90], 0)[0]
    r = rec[1].copy()
    r[BM.REC_VISITS:BM.REC_VISITS + 256] = np.full(128, 7, np.uint16).view(np.uint8)     # all equal: the first child
    first = int(r[BM.REC_LABELS:BM.REC_LABELS + 2].view(np.uint16)[0])
    assert BM.entry(r, 0)[1] == BM.canonical_label(first, BM.canonical(r[:90], 1)[1])
    r[BM.REC_COUNT] = 0
    assert BM.entry(r, 0)[1:] == (0xFFFF, 255)


def test_the_sampled_choice_in_integers():
    blabel, bgames = np.array([10, 20, 30], np.uint16), np.array([3, 1, 2], np.uint32)
    pick = lambda rnd, mg=1, al=None: BM.choose_one(blabel, bgames, 0, 3, 0, al, mg, 1, rnd)
    assert pick(0) == (10, 0)
    assert pick(0xFFFFFFFF) == (30, 2)                       # t = (2^32 - 1) * 6 >> 32 = 5: only the last running sum exceeds it
    assert pick(0x80000000) == (20, 1)                       # t = 3: the first sum above it is 4
    assert pick(0x7FFFFFFF) == (10, 0)                       # t = 2
    assert pick(0xFFFFFFFF, 2) == (30, 2) and pick(0, 2) == (10, 0) and pick(0x99999999, 2) == (10, 0)   # T = 5, t = 2
    assert pick(0x9999999A, 2) == (30, 2)                    # t = 3
    assert pick(0, 4) == (0xFFFF, -1)
    assert pick(0, 1, {20, 30}) == (20, 1) and pick(0xFFFFFFFF, 1, {10}) == (10, 0)
    assert BM.choose_one(blabel, bgames, 0, 3, 0, None, 1, 0, 0) == (10, 0)
    assert BM.choose_one(blabel, np.array([2, 5, 5], np.uint32), 0, 3, 0, None, 1, 0, 0) == (20, 1)   # the first of equals
