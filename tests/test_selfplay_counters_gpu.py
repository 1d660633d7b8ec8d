"""The lifetimes of the self-play counters on the GPU (csrc/cz_selfplay.hip): what cz_selfplay_stats, _rules_stats, _chase_stats,
_tablebase_stats and _resign_stats (with its histogram) read after games that ended in every counted way, after a second
cz_selfplay_begin on the same context, after the table set was detached, after resignation was switched on late, and with the
chase rule off.  Scripted games through `forced` labels on the constructed positions of tests/test_endings_overlap_gpu.py,
tests/test_selfplay_tablebase_gpu.py and tests/chase_cases.py; five slots at xiangqi rules, fold 3, the chase rule, resignation
at +2 (every judged mover is below it) and the set K-K, KR-K:

  0  CHASE_BOARD, CHASE_LINE         the ninth choose finds the chase: red chased, black wins, 8 plies
  1  CHASE_BOARD, the kings shuffle  the ninth choose finds the third occurrence, nobody checked or chased: a draw, 8 plies
  2  MATED, black to move            the first choose finds no king-safe move: red wins, no ply
  3  GAME_A                          the rook takes the knight: KR-K with black to move, red wins, 3 plies
  4  CHASE_BOARD, nothing forced     the first choose is judged: red resigns (black wins, no ply) — or, in a loop whose games all
                                     play on, goes on to the ply cap
"""
import numpy as np
import pytest
import torch

import chase_cases as CC
import match_model as MM
from test_endings_overlap_gpu import MATED
from test_selfplay_tablebase_gpu import GAME_A, IN_SET, _labels, tb   # noqa: F401 (tb: that module's fixture of built tables)

pytestmark = pytest.mark.gpu
SHUFFLE = ["d0d1", "e9e8", "d1d0", "e8e9"] * 2
BOARDS = np.stack([CC.CHASE_BOARD, CC.CHASE_BOARD, MATED, GAME_A[0], CC.CHASE_BOARD])
SIDES = np.array([0, 0, 1, 0, 0], np.uint8)
LINES = [CC.CHASE_LINE + CC.CHASE_LINE[:1], SHUFFLE + SHUFFLE[:1], [], GAME_A[1], []]
STEPS = 9
XQ = dict(rules="xiangqi", repetition=3, chase=True)
RESIGNED = dict(games=5, red_wins=2, black_wins=2, draws=1, plies=19, stalled=0, dropped=0, mates=1, repetitions=1, perpetuals=0,
                chases=1, tablebase=1, resigned=1, playon_games=0, playon_would_resign=0, playon_false_positives=0)


def _getters():
    from cchess_zero_amd._lib import SP_CHASE_STATS, SP_RESIGN_STATS, SP_RULES_STATS, SP_STATS, SP_TABLEBASE_STATS
    return (("cz_selfplay_stats", SP_STATS), ("cz_selfplay_rules_stats", SP_RULES_STATS), ("cz_selfplay_chase_stats", SP_CHASE_STATS),
            ("cz_selfplay_tablebase_stats", SP_TABLEBASE_STATS), ("cz_selfplay_resign_stats", SP_RESIGN_STATS))


def _read(ctx):
    """every counter through its own getter, into tensors that held 7s -> ({key: value}, histogram [64])"""
    d, hist = {}, torch.full((64,), 7, dtype=torch.int64, device="cuda")
    for name, keys in _getters():
        t = torch.full((len(keys),), 7, dtype=torch.int64, device="cuda")
        ctx.call(name, t, *([hist] if name == "cz_selfplay_resign_stats" else []))
        d.update(zip(keys, t.cpu().tolist()))
    return d, hist.cpu().numpy()


def _engine(G=len(BOARDS)):
    from cchess_zero_amd.engine import SearchEngine
    return SearchEngine(G, 1 << 12, plane_dtype=torch.float32, channels=14)


def _loop(eng, max_plies=16, **kw):
    from cchess_zero_amd.selfplay import SelfPlay
    sp = SelfPlay(eng, None, 8, exploration=False, continuous=False, max_plies=max_plies, seed=5, **kw)
    sp.start(BOARDS, SIDES, np.zeros(len(BOARDS), np.int32))
    return sp


def _play(sp, steps=STEPS, first=0):
    fwd = MM.device_forward("pos", 11)
    for t in range(first, first + steps):
        names = [line[t] if t < len(line) else None for line in LINES]
        sp.step_ply(fwd, forced=np.asarray(_labels(names), np.uint16), rand=(None, np.full(len(LINES), 0.5, np.float32)))


def _all_counters_stand(eng, dset):
    """A loop whose games all play on, max_plies 9: slots 0 .. 3 end as scripted, slot 4 is judged at every ply and ends at the
    ply cap at the latest -> the loop, every counter but `resigned` above zero and the histogram filled"""
    sp = _loop(eng, max_plies=STEPS, resign=2.0, resign_playon=1.0, tablebase=dset, **XQ)
    _play(sp)
    got, hist = _read(eng.ctx)
    assert (got["games"], got["playon_games"], got["resigned"]) == (5, 5, 0), got
    assert min(got[k] for k in ("mates", "repetitions", "chases", "tablebase", "playon_would_resign")) >= 1 and hist.sum() >= 1, (got, hist)
    return sp


def _assert_all_zero(ctx, tag):
    got, hist = _read(ctx)
    assert not any(got.values()) and not hist.any(), (tag, got, hist)


def test_the_getters_agree_with_stats_and_the_public_eight_hold_every_game(tb):   # noqa: F811
    dset = tb.device_set(IN_SET)
    eng = _engine()
    sp = _loop(eng, resign=2.0, resign_playon=0.0, tablebase=dset, **XQ)
    try:
        _play(sp)
        assert not sp.active().any()
        st = sp.stats()
        got, hist = _read(eng.ctx)
        print("getters:", got, "stats():", st)
        assert {k: got[k] for k in RESIGNED} == RESIGNED
        assert {k: st[k] for k in got if k != "sims"} == {k: got[k] for k in got if k != "sims"}      # stats() adds the searches in progress to sims
        assert got["sims"] > 0 and not hist.any() and not sp.resign_histogram().any()
        # every game, however it ended, is one of the games, one of the wins or draws, and its plies are records
        assert got["games"] == got["red_wins"] + got["black_wins"] + got["draws"] + got["stalled"]
        assert got["mates"] + got["repetitions"] + got["perpetuals"] + got["chases"] + got["tablebase"] + got["resigned"] == got["games"]
        assert len(sp.drain()) == got["plies"]
    finally:
        sp.close()
        dset.close()


@pytest.mark.parametrize("max_plies", [STEPS, 12], ids=["same_max_plies", "other_max_plies"])
def test_a_second_begin_reads_zero_before_and_after_the_setters(tb, max_plies):   # noqa: F811
    dset = tb.device_set(IN_SET)
    eng = _engine()
    sp = _all_counters_stand(eng, dset)
    try:
        ctx = eng.ctx
        ctx.call("cz_selfplay_begin", max_plies, None, None, None)
        _assert_all_zero(ctx, "begun")
        ctx.call("cz_selfplay_set_rules", 1)
        ctx.call("cz_selfplay_set_repetition", 3)
        ctx.call("cz_selfplay_set_chase", 1)
        ctx.call("cz_selfplay_set_resign", 2.0, 0, 1.0, 5)
        ctx.call("cz_selfplay_set_tablebase", dset.h)
        _assert_all_zero(ctx, "set")
    finally:
        sp.close()
        dset.close()


def test_detaching_keeps_the_tablebase_count_and_attaching_goes_on_from_it(tb):   # noqa: F811
    from cchess_zero_amd.selfplay import SelfPlay
    dset = tb.device_set(IN_SET)
    eng = _engine(1)
    sp = SelfPlay(eng, None, 4, exploration=False, continuous=True, rules="xiangqi", tablebase=dset)
    sp.start(GAME_A[0][None], np.zeros(1, np.uint8), np.zeros(1, np.int32))

    def step(name):
        sp.step_ply(MM.device_forward("pos", 11), forced=np.asarray(_labels([name]), np.uint16), rand=(None, np.full(1, 0.5, np.float32)))
        return sp.fin_n.cpu().tolist(), _read(eng.ctx)[0]["tablebase"], sp.stats()["tablebase"]

    try:
        assert [step(m) for m in GAME_A[1]] == [([0], 0, 0), ([0], 0, 0), ([3], 1, 1)]
        sp.set_tablebase(None)                    # the slot's second game, from the same start, with no set: it goes on
        assert [step(m) for m in GAME_A[1]] == [([0], 1, 1)] * 3
        sp.set_tablebase(dset)                    # it sits in a covered position, and is judged after its next move
        assert step("e8e9") == ([4], 2, 2)
    finally:
        sp.close()
        dset.close()


def test_resignation_switched_on_late_starts_from_zeros(tb):   # noqa: F811
    dset = tb.device_set(IN_SET)
    eng = _engine()
    _all_counters_stand(eng, dset).close()
    sp = _loop(eng, resign_playon=0.0, **XQ)         # the same context, resignation off
    try:
        _play(sp, 1)                                  # slot 2 is mated, slot 4 plays a move of its own
        st = sp.stats()
        assert st["games"] == st["mates"] == 1 and "resigned" not in st
        sp.set_resign_threshold(2.0)
        st = sp.stats()
        assert [st[k] for k in ("resigned", "playon_games", "playon_would_resign", "playon_false_positives")] == [0] * 4
        assert not sp.resign_histogram().any() and not _read(eng.ctx)[1].any()
        _play(sp, 1, first=1)                         # slot 4 is judged now: black, to move, resigns a game of one ply
        st = sp.stats()
        assert (st["games"], st["resigned"], st["red_wins"], st["plies"], st["playon_games"]) == (2, 1, 2, 1, 0)
    finally:
        sp.close()
        dset.close()


def test_the_chase_getter_reads_zero_with_the_rule_off(tb):   # noqa: F811
    dset = tb.device_set(IN_SET)
    eng = _engine()
    _all_counters_stand(eng, dset).close()
    sp = _loop(eng, rules="xiangqi", repetition=3)   # the same context, the chase rule off: the chase line is a draw by repetition
    try:
        assert _read(eng.ctx)[0]["chases"] == 0
        _play(sp)
        got, _ = _read(eng.ctx)
        assert got["chases"] == 0 and got["repetitions"] >= 2 and "chases" not in sp.stats(), got
    finally:
        sp.close()
        dset.close()
