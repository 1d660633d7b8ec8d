"""Tablebase adjudication in self-play on the GPU (cz_selfplay_set_tablebase, csrc/cz_selfplay.hip; SelfPlay(tablebase=...)):
scripted games through `forced` labels, so that nothing depends on the net; what must happen comes from
tests/tablebase_set_model.py on the recorded tables (tests/golden/tablebase_model.npz)."""
import numpy as np
import pytest
import torch

import kingsafe_model as KM
import match_model as MM
import tablebase_model as TM
import tablebase_set_model as SM

pytestmark = pytest.mark.gpu
NONE = 0xFFFF
IN_SET = ["K-K", "KR-K"]      # KN-K is loaded too, and left out of the set
LEVELS = [dict(), dict(repetition=3), dict(repetition=3, chase=True)]


@pytest.fixture(scope="module")
def tb():
    from cchess_zero_amd.tablebase import Tablebase
    t = Tablebase()
    for s in ("KR-K", "KN-K"):
        t.build(s)
    values, _ = TM.golden()
    for s in ("K-K", "KR-K", "KN-K"):
        assert np.array_equal(t.tables[s].cpu().numpy(), values[s])
    return t


def _labels(names):
    from cchess_zero_amd._lib import tables
    l2i = tables()["label2i"]
    return [NONE if n is None else int(l2i[n]) for n in names]


def _place(**pieces):
    """squares by ICCS name -> a board: _place(e0=1, a4=3)"""
    b = np.zeros(90, np.uint8)
    for sq, code in pieces.items():
        b[9 * int(sq[1]) + "abcdefghi".index(sq[0])] = code
    return b


# (a) two quiet plies, then the rook takes the knight: KR-K with black to move, a loss for black
GAME_A = (_place(d0=1, a4=3, e9=8, a8=12), ["d0d1", "e9e8", "a4a8"])
# (b) the king takes the rook that checks it: K-K, a draw.  (c) the knight takes the pawn: KN-K, which the set does not hold
GAME_B = (_place(e0=1, e1=10, f9=8), ["e0e1"])
GAME_C = (_place(d0=1, c2=5, d4=13, e9=8), ["c2d4", "e9e8", "d0d1"])


def _replay(board, names, side=0):
    """-> the positions [(board, side to move)] before every move and after the last; every move is asserted king-safe"""
    from cchess_zero_amd._lib import tables
    srcdst = tables()["srcdst"]
    out, b = [(board.copy(), side)], board.copy()
    for lab in _labels(names):
        assert lab in set(KM.kingsafe(b, side)[0].tolist()), (names, lab)
        b = b.copy()
        src, dst = int(srcdst[lab]) & 0xFF, int(srcdst[lab]) >> 8
        b[dst], b[src] = b[src], 0
        side ^= 1
        out.append((b, side))
    return out


def _selfplay(boards, playouts=4, **kw):
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    boards = np.asarray(boards, np.uint8).reshape(-1, 90)
    eng = SearchEngine(len(boards), 1 << 12, plane_dtype=torch.float32, channels=14)
    sp = SelfPlay(eng, None, playouts, exploration=False, rules="xiangqi", **kw)
    sp.start(boards, np.zeros(len(boards), np.uint8), np.zeros(len(boards), np.int32))
    return eng, sp


def _step(sp, names):
    sp.step_ply(MM.device_forward("pos", 11), forced=np.asarray(_labels(names), np.uint16), rand=(None, np.full(len(names), 0.5, np.float32)))
    return sp.fin_n.cpu().tolist()


def _model_end(values, line):
    """(how, loser) at the adjudicate behind the last move of a replayed line, with IN_SET attached"""
    b, side = line[-1]
    v, _ = SM.probe(values, IN_SET, b, side)
    return SM.verdict(v, side, red_king=bool((b == 1).any()), black_king=bool((b == 8).any()), ply=len(line) - 1, max_plies=512)


@pytest.mark.parametrize("level", LEVELS, ids=["kingsafe", "repetition", "chase"])
def test_three_scripted_games(tb, level):
    from cchess_zero_amd.selfplay import unpack_records
    values, _ = TM.golden()
    la, lb, lc = _replay(*GAME_A), _replay(*GAME_B), _replay(*GAME_C)
    # what the model says: (a) ends after its third move as a loss for black, (b) after its first as a draw, (c) goes on; and no
    # position before those is covered
    assert _model_end(values, la) == (SM.TABLEBASE, 1) and _model_end(values, lb) == (SM.TABLEBASE, -1) and _model_end(values, lc)[0] == 0
    assert all(_model_end(values, la[:k + 1])[0] == 0 for k in (1, 2)) and all(_model_end(values, lc[:k + 1])[0] == 0 for k in (1, 2, 3))
    assert TM.signature_of(lc[1][0]) == "KN-K" and "KN-K" in tb.tables
    dset = tb.device_set(IN_SET)
    eng, sp = _selfplay([GAME_A[0], GAME_B[0], GAME_C[0]], tablebase=dset, **level)
    try:
        # the slot of (b) is re-seeded after its first ply: its next game plays two quiet plies
        assert _step(sp, ["d0d1", "e0e1", "c2d4"]) == [0, 1, 0]
        root = eng.root_state()
        assert np.array_equal(root[0].cpu().numpy()[1], GAME_B[0]) and int(root[1][1]) == 0      # re-seeded: its start position, red to move
        assert _replay(GAME_B[0], ["e0d0", "e1e5"])
        assert _step(sp, ["e9e8", "e0d0", "e9e8"]) == [0, 0, 0]
        assert _step(sp, ["a4a8", "e1e5", "d0d1"]) == [3, 0, 0]
        root = eng.root_state()
        assert np.array_equal(root[0].cpu().numpy()[0], GAME_A[0]) and int(root[1][0]) == 0
        assert np.array_equal(root[0].cpu().numpy()[2], lc[3][0])                                  # (c) went on
        u = unpack_records(sp.drain())
        assert u["side"].tolist() == [0, 0, 1, 0] and u["ply"].tolist() == [0, 0, 1, 2]
        assert u["z"].tolist() == [0, 1, -1, 1]                  # (b): a draw; (a): black, the side to move at the end, lost
        assert np.array_equal(u["boards"][0], GAME_B[0]) and all(np.array_equal(u["boards"][1 + k], la[k][0]) for k in range(3))
        st = sp.stats()
        assert (st["games"], st["red_wins"], st["black_wins"], st["draws"], st["plies"], st["stalled"], st["tablebase"]) == (2, 1, 0, 1, 4, 0, 2)
        assert (st["mates"], st["repetitions"], st["perpetuals"]) == (0, 0, 0)
    finally:
        sp.close()
        dset.close()


def test_black_wins_and_the_detached_set(tb):
    """The colours of (a) swapped: the black rook takes, red is to move in a lost KR-K... which is K-KR: in the set only when it is
    given.  Then the three lines with the set detached: nothing finishes."""
    from cchess_zero_amd.selfplay import unpack_records
    tb.build("K-KR")
    values = {"K-K": tb.tables["K-K"].cpu().numpy(), "K-KR": tb.tables["K-KR"].cpu().numpy()}
    start = _place(d9=8, a5=10, e0=1, a1=5)
    line = _replay(start, ["e0e1", "a5a1"])
    v, _ = SM.probe(values, ["K-K", "K-KR"], *line[-1])
    assert line[-1][1] == 0 and SM.verdict(v, 0) == (SM.TABLEBASE, 0)        # red to move has lost
    dset = tb.device_set(["K-K", "K-KR"])
    eng, sp = _selfplay([start], tablebase=dset)
    try:
        assert _step(sp, ["e0e1"]) == [0] and _step(sp, ["a5a1"]) == [2]
        assert unpack_records(sp.drain())["z"].tolist() == [-1, 1]
        st = sp.stats()
        assert (st["games"], st["red_wins"], st["black_wins"], st["draws"], st["tablebase"]) == (1, 0, 1, 0, 1)
    finally:
        sp.close()
        dset.close()
    dset = tb.device_set(IN_SET)
    eng, sp = _selfplay([GAME_A[0], GAME_B[0], GAME_C[0]], tablebase=dset)
    try:
        sp.set_tablebase(None)                                              # detached before the first ply
        assert _replay(GAME_B[0], ["e0e1", "f9f8", "e1e0"])
        assert _step(sp, ["d0d1", "e0e1", "c2d4"]) == [0, 0, 0]
        assert _step(sp, ["e9e8", "f9f8", "e9e8"]) == [0, 0, 0]
        assert _step(sp, ["a4a8", "e1e0", "d0d1"]) == [0, 0, 0]
        st = sp.stats()
        assert st["games"] == 0 and st["tablebase"] == 0 and len(sp.drain()) == 0
        sp.set_tablebase(dset)                                              # attached between two plies: (a) and (b) sit in covered positions,
        assert _step(sp, ["e8e9", "f8f9", "e8e9"]) == [4, 4, 0]            # and are judged after their next move
        assert sp.stats()["tablebase"] == 2
    finally:
        sp.close()
        dset.close()


def test_a_slot_that_did_not_move_is_not_adjudicated(tb):
    """Asynchronous plies: both slots start in a covered KR-K position; only slot 0 has had its simulations"""
    start = _place(d0=1, a4=3, e9=8)
    values, _ = TM.golden()
    assert SM.covered(SM.probe(values, IN_SET, start, 0)[0]) and _replay(start, ["a4a5"])
    dset = tb.device_set(IN_SET)
    eng, sp = _selfplay([start, start], tablebase=dset)
    try:
        fwd = MM.device_forward("pos", 11)
        forced = np.asarray(_labels(["a4a5", None]), np.uint16)
        eng.search(fwd, 4, active=np.array([1, 0], np.uint8))
        sp._transition(2, forced, (None, np.full(2, 0.5, np.float32)))          # two simulations are enough to move: slot 1 has none
        assert sp.played.cpu().numpy().view(np.uint16).tolist() == [int(forced[0]), NONE]
        assert sp.fin_n.cpu().tolist() == [1, 0]
        st = sp.stats()
        assert (st["games"], st["red_wins"], st["tablebase"]) == (1, 1, 1)
        eng.search(fwd, 4, active=np.array([0, 0], np.uint8))          # nobody moves: two covered roots, nothing ends
        sp._transition(1 << 20, None, (None, np.full(2, 0.5, np.float32)))
        assert sp.fin_n.cpu().tolist() == [0, 0] and sp.stats()["games"] == 1
    finally:
        sp.close()
        dset.close()


def test_a_set_that_covers_nothing_reachable_changes_nothing(tb):
    """Four games from the start position, six lock-step plies of a fake net, max_plies 4: with a K-K set attached the records,
    fin_n and the statistics are those of the same run without a set, byte for byte"""
    from cchess_zero_amd.rules import START_BOARD
    runs = []
    dset = tb.device_set(["K-K"])
    try:
        for with_set in (False, True):
            eng, sp = _selfplay(np.tile(np.asarray(START_BOARD, np.uint8).reshape(1, 90), (4, 1)), playouts=8, max_plies=4, repetition=3,
                                tablebase=dset if with_set else None)
            fins = []
            rng = np.random.default_rng(6)
            for _ in range(6):
                sp.step_ply(MM.device_forward("pos", 11), rand=(None, rng.random(4).astype(np.float32)))
                fins.append(sp.fin_n.cpu().tolist())
            st = sp.stats()
            assert (st.pop("tablebase") == 0) if with_set else ("tablebase" not in st)
            runs.append((sp.drain(), fins, st))
            sp.close()
    finally:
        dset.close()
    assert runs[0][0].shape[0] == 16 and np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]


def test_setter_order(tb):
    from cchess_zero_amd._lib import CchessHipError
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.selfplay import SelfPlay
    dset = tb.device_set(IN_SET)
    try:
        eng = SearchEngine(1, 1 << 10, plane_dtype=torch.float32, channels=14)
        sp = SelfPlay(eng, None, 2, exploration=False, rules="capture")
        sp.start(GAME_A[0].reshape(1, 90), np.zeros(1, np.uint8), np.zeros(1, np.int32))
        with pytest.raises(CchessHipError, match=r"cz_selfplay_set_tablebase: cz_selfplay_set_rules\(ctx, 1\) first"):
            eng.ctx.call("cz_selfplay_set_tablebase", dset.h)
        with pytest.raises(ValueError, match="tablebase needs rules='xiangqi'"):
            sp.set_tablebase(dset)
        eng.ctx.call("cz_selfplay_set_rules", 1)
        eng.ctx.call("cz_selfplay_set_tablebase", dset.h)
        with pytest.raises(CchessHipError, match=r"cz_selfplay_set_rules: the table set needs rules 1: cz_selfplay_set_tablebase\(ctx, NULL\) first"):
            eng.ctx.call("cz_selfplay_set_rules", 0)
        with pytest.raises(CchessHipError, match="cz_tb_set_destroy: the set is attached"):
            dset.close()
        assert dset.h is not None
        eng.ctx.call("cz_selfplay_set_tablebase", dset.h)          # attaching the same set again holds it once
        eng.ctx.call("cz_selfplay_set_tablebase", None)
        eng.ctx.call("cz_selfplay_set_rules", 0)                    # nothing is attached: rules 0 is accepted again
        dset.close()
        assert dset.h is None
    finally:
        dset.close()
