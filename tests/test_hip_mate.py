"""Rules.mate on the GPU against tests/mate_model.solve — status, distance and line, bit for bit: the playout corpus at 1, 3 and 5
plies in "checks" mode and the open-board subset at 3 plies in "all" mode (the model's answers are the recorded ones of
tests/golden/mate_playouts.npz, which tests/test_mate_model_cpu.py holds to a fresh run), the same answers for every slice size,
the node limit, bad roots, and the command line and the Analyzer on two mates of the corpus."""
import json

import numpy as np
import pytest

import kingsafe_model as M
import mate_model as MM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rules():
    from cchess_zero_amd.rules import Rules
    return Rules()


@pytest.fixture(scope="module")
def corpus():
    return M.playout_corpus()


@pytest.fixture(scope="module")
def model():
    return MM.playout_solutions()


def _hold(res, want, where=None):
    status, dist, pv = want
    idx = np.arange(len(status)) if where is None else where
    assert res["status"].dtype == np.uint8 and res["dist"].dtype == np.int16 and res["pv"].dtype == np.uint16 and res["nodes"].dtype == np.int64
    assert np.array_equal(res["status"], status[idx]), np.nonzero(res["status"] != status[idx])[0][:5]
    assert np.array_equal(res["dist"], dist[idx]), np.nonzero(res["dist"] != dist[idx])[0][:5]
    assert np.array_equal(res["pv"], pv[idx]), np.nonzero((res["pv"] != pv[idx]).any(axis=1))[0][:5]


@pytest.mark.parametrize("plies", MM.GOLDEN_PLIES)
def test_playout_corpus_checks_mode(rules, corpus, model, plies):
    """Every position of the corpus, the bad roots (no king, a king to take) among them: status 2 there, the model's answer on
    the 5 663 legal roots."""
    res = rules.mate(corpus[0], corpus[1], plies)
    _hold(res, model[plies])
    assert (res["status"] == MM.MATE).sum() >= (80, 105, 120)[plies // 2] and (res["status"] == MM.BAD_ROOT).sum() >= 100
    assert (res["nodes"][res["status"] == MM.BAD_ROOT] == 0).all() and (res["nodes"] >= 0).all()
    if plies == 1:       # the positions made are the checking children, nothing more
        counts = np.array([len(MM.checks(b, int(s))[0]) for b, s in zip(corpus[0][:300], corpus[1][:300])])
        legal = model[1][0][:300] != MM.BAD_ROOT
        assert np.array_equal(res["nodes"][:300][legal], counts[legal])


def test_open_boards_all_moves(rules):
    boards, side = MM.open_subset()
    sol = MM.open_solutions()
    _hold(rules.mate(boards, side, 3, attacker="all"), sol["all"])
    _hold(rules.mate(boards, side, 3, attacker="checks"), sol["checks"])
    assert ((sol["all"][1] == 3) & (sol["checks"][0] != MM.MATE)).any()          # a quiet first move among them


def test_the_slice_size_does_not_change_the_answer(rules, corpus, model):
    """chunk = 64 on the whole corpus at 5 plies (every level is cut into many slices), chunk = 1 on the 120 positions around the
    first 5-ply mates (every node a slice of its own)."""
    _hold(rules.mate(corpus[0], corpus[1], 5, chunk=64), model[5])
    deep = np.nonzero(model[5][1] == 5)[0][:3]
    idx = np.unique(np.concatenate([np.arange(max(i - 20, 0), min(i + 20, len(corpus[0]))) for i in deep]))
    res = rules.mate(corpus[0][idx], corpus[1][idx], 5, chunk=1)
    _hold(res, model[5], idx)
    assert (res["dist"] == 5).sum() >= 3
    same = rules.mate(corpus[0][idx], corpus[1][idx], 5)
    assert np.array_equal(same["nodes"], res["nodes"])


def test_node_limit(rules, corpus, model):
    """node_limit = 1: the first slice of roots is expanded (the limit is looked at before a slice, not inside it), nothing
    below it.  A root without a checking move is decided (status 0), every other root is undecided (status 3), and no mate
    is reported; with a limit nothing reaches the answers are the unlimited ones."""
    status, dist, _ = model[5]
    res = rules.mate(corpus[0], corpus[1], 5, node_limit=1)
    legal = status != MM.BAD_ROOT
    assert np.array_equal(res["status"] == MM.BAD_ROOT, ~legal)
    has_check = res["nodes"] > 0
    assert (res["status"][legal & has_check] == MM.LIMIT).all() and (res["status"][legal & ~has_check] == MM.NO_MATE).all()
    assert (status[legal & ~has_check] == MM.NO_MATE).all()                     # never a wrong answer where one is given
    assert not (res["status"] == MM.MATE).any() and (res["dist"] == MM.NONE).all() and (res["pv"] == 0xFFFF).all()
    # at 1 ply a limit that is reached after the roots' only slice changes nothing: every root is decided
    _hold(rules.mate(corpus[0], corpus[1], 1, node_limit=1), model[1])
    # a limit in the middle of the walk: what is answered as mate or no mate is the model's, the rest is status 3
    res = rules.mate(corpus[0], corpus[1], 5, chunk=256, node_limit=20000)
    decided = res["status"] != MM.LIMIT
    assert decided.any() and (~decided).any()
    assert np.array_equal(res["status"][decided], status[decided]) and np.array_equal(res["dist"][decided], dist[decided])
    assert np.array_equal(res["pv"][decided], model[5][2][decided])
    _hold(rules.mate(corpus[0], corpus[1], 5, node_limit=10 ** 9), model[5])


def test_bad_roots_and_arguments(rules, rules_golden):
    g = rules_golden
    b = g["boards"][:5].copy()
    s = g["side"][:5].copy()
    b[1, :] = 0
    b[1, :3] = 3 if s[1] == 0 else 10                     # three rooks of the side to move: refused
    b[2][b[2] == 1] = 0                                   # no red king
    b[3, :] = 0
    b[3, 4], b[3, 9 * 9 + 4], s[3] = 1, 8, 0              # the kings face each other: the mover can take the king
    res = rules.mate(b, s, 3)
    assert res["status"][1:4].tolist() == [2, 2, 2] and (res["dist"][1:4] == MM.NONE).all() and (res["pv"][1:4] == 0xFFFF).all()
    for i in (0, 4):
        st, d, pv = MM.solve(b[i], int(s[i]), 3)
        assert res["status"][i] == st and res["dist"][i] == d and np.array_equal(res["pv"][i], pv)
    empty = rules.mate(np.zeros((0, 90), np.uint8), np.zeros(0, np.uint8), 3)
    assert empty["status"].shape == (0,) and empty["pv"].shape == (0, 3)
    for plies in (0, 2, 17):
        with pytest.raises(ValueError):
            rules.mate(b, s, plies)
    with pytest.raises(ValueError):
        rules.mate(b, s, 3, attacker="some")


def test_command_line_and_analyzer_return_the_models_line(rules, corpus, model, capsys):
    from cchess_zero_amd import mate, notation
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.analysis import Analyzer
    from cchess_zero_amd.net import PolicyValueNet
    status, dist, pv = model[5]
    picks = [int(np.nonzero(dist == 3)[0][0]), int(np.nonzero(dist == 5)[0][0])]
    fens = [notation.position_to_fen(corpus[0][i], int(corpus[1][i])) for i in picks]
    names = tables()["labels"]
    lines = [[names[int(l)] for l in pv[i] if l != 0xFFFF] for i in picks]
    mate.main(["--fen", fens[0], "--fen", fens[1], "--plies", "5"], rules=rules)
    rows = [json.loads(l) for l in capsys.readouterr().out.splitlines()]
    assert [r["fen"] for r in rows] == fens and [r["status"] for r in rows] == ["mate", "mate"]
    assert [r["plies"] for r in rows] == [3, 5] and [r["mate_in"] for r in rows] == [2, 3] and [r["pv"] for r in rows] == lines
    assert all(r["nodes"] > 0 for r in rows)
    an = Analyzer(PolicyValueNet(res_block_nums=1, seed=3), 16, 2)
    res = an.analyse(fens + [notation.START_FEN], mate_plies=5)
    assert [r["mate"] for r in res] == [dict(plies=3, pv=lines[0]), dict(plies=5, pv=lines[1]), None]
    plain = an.analyse(fens + [notation.START_FEN])
    assert all("mate" not in r for r in plain)
    for a, b in zip(res, plain):                          # the search result itself is unchanged
        assert {k: v for k, v in a.items() if k != "mate"} == b
