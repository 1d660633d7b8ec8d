"""Perft under Xiangqi rules on the CPU: tests/golden/perft.json (written by tests/golden/gen_perft.py; the start position's
node row is the PUBLISHED Xiangqi perft table, 44, 1 920, 79 666, 3 290 240, 133 312 995, 5 392 831 844) against

  1. the host perft (tests/perft_host.cpp: a recursion over cz_kingsafe.h, the function cz_movegen_kingsafe runs per lane):
     the start position to depth 4, all four columns, and every other position of the fixture to its own depth;
  2. an implementation that shares nothing with that header (tests/perft_model.py: kingsafe_model's moves over the C oracle's
     pseudo-legal generator, a numpy make-move): the start position to depth 3, every other position to depth 2.

The published table is what anchors the king-safe definition outside this repository; tests/test_hip_perft.py carries it to the
device."""
import json
import os

import numpy as np
import pytest

import perft_host
import perft_model

COLUMNS = perft_host.COLUMNS


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return json.load(open(os.path.join(golden_dir, "perft.json")))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return perft_host.load(tmp_path_factory.mktemp("perft"))


def _rows(entry, depth):
    return {k: entry[k][:depth + 1] for k in COLUMNS}


def _as_lists(t):
    return {k: [int(x) for x in t[k]] for k in COLUMNS}


def test_fixture_holds_the_published_table_and_a_corpus_that_is_not_trivial(fixture):
    s = fixture["start"]
    assert s["nodes"] == [1, 44, 1920, 79666, 3290240, 133312995] and s["nodes_depth6"] == 5392831844
    assert s["captures"] == [0, 2, 72, 3159, 115365, 4917734] and s["checks"] == [0, 0, 6, 384, 19380, 953251] and s["mates"] == [0, 0, 0, 0, 0, 584]
    P = fixture["positions"]
    assert len(P) >= 12
    assert sum(p["checks"][0] for p in P) >= 3 and any(p["side"] == 1 for p in P) and any(p["tag"] == "flying" for p in P)
    assert any(p["mates"][0] == 1 and p["nodes"] == [1] + [0] * p["depth"] for p in P)
    assert all(sum(sum(p[k][1:]) for p in P) > 0 for k in ("captures", "checks", "mates"))
    assert all(p["depth"] == (2 if p["tag"] == "open" else 3) for p in P) and sum(p["tag"] == "open" for p in P) >= 3


def test_host_perft_start_position_depth_4(host, fixture):
    s = fixture["start"]
    assert _as_lists(host(s["board"], s["side"], 4)) == _rows(s, 4)
    assert [int(x) for x in host(s["board"], s["side"], 4, stats=False)["nodes"]] == s["nodes"][:5]   # the last ply counted, not made


def test_host_perft_every_other_position(host, fixture):
    for p in fixture["positions"]:
        assert _as_lists(host(p["board"], p["side"], p["depth"])) == _rows(p, p["depth"]), p["source"]
        assert [int(x) for x in host(p["board"], p["side"], p["depth"], stats=False)["nodes"]] == p["nodes"], p["source"]


def test_model_perft_start_position_depth_3(fixture):
    s = fixture["start"]
    assert _as_lists(perft_model.perft(s["board"], s["side"], 3)) == _rows(s, 3)


def test_model_perft_every_other_position_depth_2(fixture):
    for p in fixture["positions"]:
        assert _as_lists(perft_model.perft(p["board"], p["side"], 2)) == _rows(p, 2), p["source"]


def test_model_successors_is_the_contract():
    """perft_model.successors, the model tests/test_hip_perft.py holds cz_successors to, on a batch small enough to read: order,
    offsets, a refused parent (count 0xFFFF) and a parent without moves have no children, a capture is reported."""
    from oracle import oracle as O
    b = O.fen_to_board(O.START_FEN)
    pseudo = O.legal_moves(b, 0)
    moves = np.full((3, 128), 0xFFFF, np.uint16)
    moves[0, :len(pseudo)] = pseudo
    moves[2, :2] = pseudo[:2]
    cb, cs, cap, par, lab, off = perft_model.successors(np.stack([b, b, b]), [0, 1, 1], moves, np.array([len(pseudo), 0xFFFF, 2], np.uint16))
    assert list(off) == [0, len(pseudo), len(pseudo), len(pseudo) + 2] and len(cb) == len(pseudo) + 2
    assert list(par) == [0] * len(pseudo) + [2, 2] and list(lab) == list(pseudo) + list(pseudo[:2]) and list(cs) == [1] * len(pseudo) + [0, 0]
    for j, m in enumerate(pseudo):
        nb, taken = O.apply_move(b, int(m))[:2]
        assert np.array_equal(cb[j], nb) and int(cap[j]) == int(b[int(O.label_srcdst()[m]) >> 8])
    assert (cap != 0).sum() == 2     # the two cannon captures of the start position
