"""tests/tablebase_model.py on the CPU: the committed tables (tests/golden/tablebase_model.npz) are what a fresh run of the model
gives on the small signatures, and the facts of the model that the kernels' tests lean on."""
import numpy as np
import pytest

import tablebase_model as TM

FRESH = ("K-K", "K-KA", "KP-K", "KN-K")


@pytest.fixture(scope="module")
def golden():
    return TM.golden()


@pytest.fixture(scope="module")
def fresh():
    done = {}
    for s in FRESH:
        TM.build_closure(s, done)
    return done


def test_the_definitions():
    assert [len(TM.domain(c, b)) for c in "KABPRNC" for b in (0, 1)] == [9, 9, 5, 5, 7, 7, 55, 55, 90, 90, 90, 90, 90, 90]
    assert list(TM.domain("A", 1)) == [66, 68, 76, 84, 86] and list(TM.domain("B", 1)) == [47, 51, 63, 67, 71, 83, 87]
    assert list(TM.domain("P", 0)[:11]) == [27, 29, 31, 33, 35, 36, 38, 40, 42, 44, 45] and list(TM.domain("P", 1)[44:]) == [44, 45, 47, 49, 51, 53, 54, 56, 58, 60, 62]
    assert TM.entries("K-K") == 162 and TM.entries("KR-KAA") == 364500 and TM.entries("KP-KP") == 490050
    assert TM.closure("KR-KAA") == ["K-K", "K-KA", "K-KAA", "KR-K", "KR-KA", "KR-KAA"]
    assert TM.sub_signature("KR-KAA", 1) == "K-KAA" and TM.sub_signature("KR-KAA", 3) == "KR-KA" == TM.sub_signature("KR-KAA", 4)
    for bad in ("", "K", "K-", "R-K", "KK-K", "KRK-K", "KAR-K", "KRRR-K", "KPPPPPP-K", "K-K-K", "KX-K", "k-k"):
        with pytest.raises(ValueError):
            TM.parse(bad)
    # index = 2 * mixed radix + side, slot 0 the most significant digit
    board, side = TM.unrank("KR-KAA", 2 * (((4 * 90 + 7) * 9 + 8) * 5 + 1) * 5 + 2 * 3 + 1)
    assert side == 1 and board[13] == 1 and board[7] == 3 and board[86] == 8 and board[68] == 9 and board[84] == 9 and (board != 0).sum() == 5
    # the k-th of equal pieces in ascending square order stands on the k-th slot: the swapped index ranks to the canonical one
    swapped = 2 * (((4 * 90 + 7) * 9 + 8) * 5 + 3) * 5 + 2 * 1 + 1
    assert np.array_equal(TM.unrank("KR-KAA", swapped)[0], board) and TM.rank("KR-KAA", board, 1) != swapped
    assert TM.unrank("KR-KAA", TM.rank("KR-KAA", board, 1))[1] == 1
    assert TM.unrank("KR-KAA", 2 * (((4 * 90 + 13) * 9 + 8) * 5 + 1) * 5 + 2 * 3)[0] is None       # the rook on the king's square
    assert TM.rank("KR-KAA", TM.unrank("KN-KA", 4242)[0], 0) is None


@pytest.mark.parametrize("sig", list(FRESH))
def test_golden_file_is_a_fresh_run(golden, fresh, sig):
    values, passes = golden
    assert values[sig].dtype == np.int16 and np.array_equal(values[sig], fresh[sig].values) and passes[sig] == fresh[sig].passes


def test_golden_file_has_every_table_the_tests_read(golden):
    values, passes = golden
    want = set()
    for s in TM.GOLDEN_TABLES:
        want |= set(TM.closure(s))
    assert set(values) == want == set(passes)
    for s in values:
        assert values[s].shape == (TM.entries(s),)


def test_model_facts(golden, fresh):
    values, passes = golden
    kck = values["KC-K"]
    assert ((kck == 0) | (kck == TM.ILLEGAL)).all() and passes["KC-K"] == 1                   # a lone cannon decides nothing
    for s, v in values.items():
        v = v.astype(np.int64)
        legal = v != TM.ILLEGAL
        assert (v != TM.UNKNOWN).all() and (v != TM.MISS).all()
        assert ((v[legal & (v > 0)] - 1) % 2 == 1).all() and ((-v[legal & (v < 0)] - 1) % 2 == 0).all(), s   # wins are odd, losses even
    # red's and black's pawn endings mirror each other
    assert sorted(values["KP-K"].tolist()) == sorted(values["K-KP"].tolist())
    # no index has an ILLEGAL child, and every value is the pass rule on its children's final values
    for s in ("KP-K", "KN-K"):
        t = fresh[s]
        u = np.zeros(len(t.child_idx), np.int64)
        for k, name in enumerate(t.tabs):
            u[t.child_tab == k] = fresh[name].values[t.child_idx[t.child_tab == k]]
        assert (u != TM.ILLEGAL).all()
        for j in range(0, len(t.parents), 37):
            c = u[t.offsets[j]:t.offsets[j + 1]]
            v = int(t.values[t.parents[j]])
            want = int(TM.plies(c[c < 0]).min()) + 2 if (c < 0).any() else -(int(TM.plies(c).max()) + 2) if (c > 0).all() else 0
            assert v == want, (s, j)


def test_the_recorded_kp_kp_is_the_one_of_the_full_stop_rule(fresh):
    """KP-KP's sub-tables hold losses of 20 plies, so captures settle parents up to pass 21: the recorded table (the model takes
    minutes on it, so it is only read here) has the 13 362 wins and the 21-ply win of the full stop rule, where "the first empty
    pass" alone stops at 8 538 wins of at most 11 plies"""
    sub = fresh["KP-K"].stats()
    assert sub["longest_loss"] == 20 and sub["passes"] == 21
    values, passes = TM.golden()
    v = values["KP-KP"].astype(np.int64)
    win = (v > 0) & (v != TM.UNKNOWN)
    assert int(win.sum()) == 13362 and int(v[win].max()) - 1 == 21 and passes["KP-KP"] == 22
