"""tests/mate_model.py against itself (no GPU, no kernel): the lines it reports are mates, its horizons agree with each other,
its corpora hold enough mates to mean something, and the recorded answers the GPU tests read (tests/golden/mate_playouts.npz)
are what a fresh run of the model gives."""
import numpy as np
import pytest

import kingsafe_model as M
import mate_model as MM
from perft_model import make_move


@pytest.fixture(scope="module")
def corpus():
    return M.playout_corpus()


@pytest.fixture(scope="module")
def fresh(corpus):
    """solve() in "checks" mode on every position of the playout corpus at 1, 3 and 5 plies (~50 s)"""
    return {p: MM.solve_batch(corpus[0], corpus[1], p) for p in MM.GOLDEN_PLIES}


@pytest.fixture(scope="module")
def open_fresh():
    boards, side = MM.open_subset()
    return boards, side, {m: MM.solve_batch(boards, side, 3, m) for m in ("all", "checks")}


def _same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def test_the_recorded_answers_are_the_models(fresh, open_fresh):
    rec = MM.playout_solutions()
    for p in MM.GOLDEN_PLIES:
        assert _same(rec[p], fresh[p]), p
    rec = MM.open_solutions()
    for m in ("all", "checks"):
        assert _same(rec[m], open_fresh[2][m]), m


def _check_lines(boards, side, sol, checks_only):
    status, dist, pv = sol
    n = 0
    for i in np.nonzero(status == MM.MATE)[0]:
        b, s = boards[i], int(side[i])
        line = [int(l) for l in pv[i] if l != 0xFFFF]
        assert len(line) == dist[i] and dist[i] % 2 == 1 and (pv[i, len(line):] == 0xFFFF).all(), i
        for k, l in enumerate(line):
            if k % 2 == 0 and checks_only:
                assert l in MM.checks(b, s)[0], (i, k)          # every attacker move is a check
            else:
                assert l in M.kingsafe(b, s)[0], (i, k)
            b, s = make_move(b, l)[0], 1 - s
        assert M.kingsafe(b, s)[1] & M.NO_SAFE_MOVE, i          # the line ends in a position without a king-safe move
        if checks_only:
            assert M.kingsafe(b, s)[1] & M.IN_CHECK, i
        n += 1
    assert ((status != MM.MATE) == (dist == MM.NONE)).all() and (pv[status != MM.MATE] == 0xFFFF).all()
    return n


def test_every_line_is_a_mate_and_every_attacker_move_a_check(corpus, fresh, open_fresh):
    for p in MM.GOLDEN_PLIES:
        assert _check_lines(corpus[0], corpus[1], fresh[p], True) >= 80
    assert _check_lines(open_fresh[0], open_fresh[1], open_fresh[2]["checks"], True) >= 1
    assert _check_lines(open_fresh[0], open_fresh[1], open_fresh[2]["all"], False) >= 1


def test_a_deeper_horizon_keeps_the_shorter_mates(fresh):
    """Distances within the horizon are exact shortest mates whatever the horizon: solve(5) agrees with solve(3), and solve(3)
    with solve(1), in distance and line wherever the shallower one finds a mate; what the deeper one adds is longer."""
    for lo, hi in ((1, 3), (3, 5)):
        s0, d0, p0 = fresh[lo]
        s1, d1, p1 = fresh[hi]
        found = s0 == MM.MATE
        assert found.any() and (s1[found] == MM.MATE).all() and np.array_equal(d1[found], d0[found])
        assert np.array_equal(p1[found][:, :lo], p0[found]) and (p1[found][:, lo:] == 0xFFFF).all()
        assert (d1[(s1 == MM.MATE) & ~found] == hi).all()
        assert np.array_equal(s0 == MM.BAD_ROOT, s1 == MM.BAD_ROOT)


def test_the_playout_corpus_holds_mates_of_every_length(corpus, fresh):
    """Measured with this model over the 5 663 legal roots of the 6 272 positions: 100 mates in 1 ply, 33 in 3, 23 in 5."""
    status, dist, _ = fresh[5]
    legal = MM.legal_roots(*corpus)
    assert len(legal) >= 5000 and np.array_equal(np.nonzero(status != MM.BAD_ROOT)[0], legal)
    counts = [int((dist == d).sum()) for d in (1, 3, 5)]
    print("playout corpus: %d legal roots, mates in 1 / 3 / 5 plies: %s" % (len(legal), counts))
    assert counts[0] >= 80 and counts[1] >= 25 and counts[2] >= 15


def test_all_moves_finds_mates_that_checks_alone_do_not(open_fresh):
    """The open-board subset (71 roots), 3 plies.  Measured: "all" mode 34 mates in 1 ply and 23 in 3; "checks" mode 30 in 1 ply
    and 16 in 3; 8 roots have a 3-ply mate in "all" mode and no mate in "checks" mode (a quiet first move), 4 a 1-ply mate that
    is no check: stalemate, which loses too.  The model takes ~25 s for both modes."""
    boards, side, sol = open_fresh
    (sa, da, _), (sc, dc, _) = sol["all"], sol["checks"]
    print("open subset: %d roots; all: %d in 1 ply, %d in 3; checks: %d in 1 ply, %d in 3; quiet 3-ply mates %d, stalemates in 1 %d"
          % (len(boards), (da == 1).sum(), (da == 3).sum(), (dc == 1).sum(), (dc == 3).sum(), ((da == 3) & (sc != MM.MATE)).sum(), ((da == 1) & (dc != 1)).sum()))
    assert len(boards) >= 40
    assert ((da == 3) & (sc != MM.MATE)).sum() >= 1                 # a 3-ply mate that "checks" mode does not find
    found = sc == MM.MATE
    assert (sa[found] == MM.MATE).all() and (da[found] <= dc[found]).all()      # every check is a move: "all" is never slower


def test_backup_by_hand():
    """offsets 0 3 3 5 6: parent 0 has (4, 2, 2), parent 1 none, parent 2 (NONE, 6), parent 3 (NONE)"""
    off = np.array([0, 3, 3, 5, 6], np.int32)
    dist = np.array([4, 2, 2, MM.NONE, 6, MM.NONE], np.int16)
    label = np.array([10, 11, 12, 13, 14, 15], np.uint16)
    pv = np.array([[100, 0xFFFF], [101, 201], [102, 202], [103, 203], [104, 0xFFFF], [105, 205]], np.uint16)
    d, line = MM.backup(off, 6, dist, label, pv, 2, 0)
    assert d.tolist() == [3, MM.NONE, 7, MM.NONE]
    assert line.tolist() == [[11, 101, 201], [0xFFFF] * 3, [14, 104, 0xFFFF], [0xFFFF] * 3]
    d, line = MM.backup(off, 6, dist, label, pv, 2, 1)
    assert d.tolist() == [5, 0, MM.NONE, MM.NONE]
    assert line.tolist() == [[10, 100, 0xFFFF], [0xFFFF] * 3, [0xFFFF] * 3, [0xFFFF] * 3]
    d, line = MM.backup(off, 2, dist, label, None, 0, 0)            # total = 2: parent 0 keeps two children, the others none
    assert d.tolist() == [3, MM.NONE, MM.NONE, MM.NONE] and line.tolist() == [[11], [0xFFFF], [0xFFFF], [0xFFFF]]
