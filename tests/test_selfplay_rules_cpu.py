"""Self-play under Xiangqi rules without a GPU: the new C ABI is declared, exported and bound; the host model of
tests/selfplay_rules_model.py on constructed positions (two mates in one, a perpetual check, a quiet shuffle); SelfPlay's
argument validation."""
import ctypes
import os
import re

import numpy as np
import pytest

import kingsafe_model as KM
import repetition_cases as RC
import repetition_model as RM
import selfplay_rules_model as XS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cz_selfplay_set_rules", "cz_selfplay_set_repetition", "cz_selfplay_history", "cz_selfplay_rules_stats")
QUIET_LINE = ["e5e4", "d9d8", "e4e5", "d8d9"]


def _board(fen):
    from oracle import oracle as O
    return O.fen_to_board(fen)


def _labels(names):
    from oracle import oracle as O
    lab = O.labels()
    return [lab.index(n) for n in names]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__
    __graft_entry__.build_hip_only()
    from cchess_zero_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cchess_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cz_[a-z_0-9]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in declared, n
        assert hasattr(L, n), "symbol %s is not exported" % n
        assert n in _lib.EXPORTS, n
    assert _lib.SP_RULES_STATS == ("mates", "repetitions", "perpetuals") and len(_lib.SP_STATS) == 8


# ---- the model on constructed positions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fen,side,move", [("4K4/8r/9/9/9/r8/9/9/9/3k5", 1, "a5a0"), ("3K5/9/9/9/R8/9/9/9/8R/4k4", 0, "a4a9")])
def test_mate_in_one(fen, side, move):
    from oracle import oracle as O
    b = _board(fen)
    mv = _labels([move])[0]
    assert mv in set(KM.kingsafe(b, side)[0].tolist())
    nb = O.apply_move(b, mv)[0]
    assert (nb == 1).any() and (nb == 8).any()
    safe, flags = KM.kingsafe(nb, 1 - side)
    assert len(O.legal_moves(nb, 1 - side)) == 3 and len(safe) == 0 and flags == KM.IN_CHECK | KM.NO_SAFE_MOVE
    # the model's choice finds no child, and its adjudication gives the game to the side that mated
    lab = O.legal_moves(nb, 1 - side)
    pick, _, idx = XS.choose_xq_ref(nb, 1 - side, lab, np.ones(len(lab), np.int64), 1.0, None, 0.0, 0.5)
    assert pick is None and idx == []
    o = XS.adjudicate_xq_ref(RM.NONE, True, 1 - side, nb, 1, 1, [side], 512)
    assert (o.result, o.how, o.fin_n, o.z.tolist()) == ("black" if side else "red", "mate", 1, [1])


def test_perpetual_check_is_a_loss_for_red_at_ply_8():
    line = _labels(RC.PERPETUAL_LINE) * 3
    h = XS.replay_line(RC.perpetual_board(), 0, line, fold=3)
    assert (h["ply"], h["code"], h["first"]) == (8, RM.RED_LOSES, 0)
    assert h["safe"] and h["captures"] == 0
    movers = [i & 1 for i in range(8)]
    o = XS.adjudicate_xq_ref(h["code"], False, 0, None, 0, 8, movers, 512)
    assert (o.result, o.how, o.fin_n) == ("black", "perpetual", 8) and o.z.tolist() == [-1, 1] * 4


def test_quiet_shuffle_is_a_draw_at_ply_8():
    line = _labels(QUIET_LINE) * 3
    h = XS.replay_line(RC.perpetual_board(), 0, line, fold=3)
    assert (h["ply"], h["code"]) == (8, RM.DRAW)
    assert h["safe"] and h["captures"] == 0 and not any(h["checks"])
    o = XS.adjudicate_xq_ref(h["code"], False, 0, None, 0, 8, [i & 1 for i in range(8)], 512)
    assert (o.result, o.how, o.fin_n) == ("draw", "repetition", 8) and not o.z.any()


def test_ending_order_repetition_then_mate_then_the_rest():
    b = _board("4K4/9/9/9/9/9/9/9/9/3k5")
    assert XS.adjudicate_xq_ref(RM.DRAW, True, 0, b, 60, 3, [0, 1, 0], 512).how == "repetition"
    assert XS.adjudicate_xq_ref(RM.NONE, True, 0, b, 60, 3, [0, 1, 0], 512).how == "mate"
    o = XS.adjudicate_xq_ref(RM.NONE, False, 0, b, 60, 3, [0, 1, 0], 512)
    assert o.how is None and o.result == "draw"
    assert XS.adjudicate_xq_ref(RM.NONE, False, 0, b, 0, 3, [0, 1, 0], 512) is None
    # fin_n = min(ply, max_plies)
    assert XS.adjudicate_xq_ref(RM.BLACK_LOSES, False, 0, b, 0, 5, [0, 1, 0, 1, 0], 4).z.tolist() == [1, -1, 1, -1]


def test_a_record_whose_king_safe_children_have_no_visit_is_a_uniform_pi():
    """Every simulation of a short search can go to children that are not king-safe: the record then holds k children with
    zero visits.  The choose kernel plays uniformly from it (wave_visit_policy), and to_dense gives 1 / k — not the NaN of
    softmax(log 0)."""
    from cchess_zero_amd.selfplay import pack_records, to_dense
    b = _board("4K4/9/9/4R4/9/9/9/9/4r4/3k5")
    safe = KM.kingsafe(b, 0)[0]
    lab = np.full((2, 128), 0xFFFF, np.uint16)
    lab[:, :len(safe)] = safe
    vis = np.zeros((2, 128), np.int64)
    vis[1, 2] = 5
    rec = pack_records(np.stack([b, b]), np.zeros(2), lab, vis, np.full(2, len(safe)), np.zeros(2))
    for exact in (True, False):
        pi = to_dense(rec, 1.0, exact=exact)[1]
        assert np.isfinite(pi).all() and np.array_equal(pi[0, safe], np.full(len(safe), 1.0 / len(safe))) and pi[0].sum() == pytest.approx(1.0, abs=1e-15)
        assert pi[1, safe[2]] == 1.0 and pi[1].sum() == 1.0


# ---- arguments ------------------------------------------------------------------------------------------------------------
def test_selfplay_validates_rules_and_repetition():
    from cchess_zero_amd.selfplay import SelfPlay
    for kw in (dict(rules="chess"), dict(rules="xiangqi", repetition=1), dict(repetition=3), dict(rules="capture", repetition=3),
               dict(rules="xiangqi", repetition=9), dict(rules="xiangqi", repetition=True)):
        with pytest.raises(ValueError):
            SelfPlay(None, None, 8, **kw)
