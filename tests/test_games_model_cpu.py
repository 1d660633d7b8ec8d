"""tests/games_model.py, the model of cz_games_replay, on the reference's own six self-play games (tests/golden/selfplay.npz):
every record the model writes carries the board, the count and the list the UNMODIFIED reference recorded for that ply, so the
reference itself anchors the model that the kernel, the host build and games.py are held to.  The figures below were computed
by this model and are kept as literals."""
import numpy as np

import games_model as GM


def _unflip_states(g, rows):
    """the fixture's states are canonical (try_flip for black, which is an involution): back to real coordinates"""
    from cchess_zero_amd.selfplay import canonical_boards
    return canonical_boards(g["state"][rows], g["side"][rows])


def test_the_six_reference_games_replay_completely_under_capture_rules():
    from cchess_zero_amd.selfplay import unpack_records
    moves, lens, results, rows, g = GM.golden_games()
    out = GM.replay(None, None, moves, lens, results, 0)
    assert out["valid"].tolist() == [35, 223, 52, 1, 13, 18] and lens.tolist() == out["valid"].tolist()
    assert (out["status"] == GM.OK).all() and out["total"] == 342
    u = unpack_records(out["records"])
    allrows = np.concatenate(rows)
    assert np.array_equal(u["boards"], _unflip_states(g, allrows)) and np.array_equal(u["side"], g["side"][allrows])
    assert np.array_equal(u["counts"], g["count"][allrows])
    k = np.arange(128)[None, :] < g["count"][allrows][:, None]
    assert np.array_equal(u["labels"][k], g["labels"][allrows][k]) and (u["labels"][~k] == 0xFFFF).all()
    assert np.array_equal(u["z"].astype(np.float64), g["z"][allrows]) and (u["flags"] == 0).all()
    assert np.array_equal(u["ply"], np.concatenate([np.arange(len(r)) for r in rows]))
    played = u["labels"][np.arange(342), u["visits"].argmax(axis=1)]
    assert np.array_equal(played, g["played"][allrows]) and (u["visits"].sum(axis=1) == 1).all()
    gone = (out["end_flags"] & (GM.RED_KING_GONE | GM.BLACK_KING_GONE)) != 0
    assert gone.tolist() == [True, True, True, False, True, True]          # five of the six end with a king taken
    # the winner is the side whose king stands
    for c in range(6):
        if gone[c]:
            assert results[c] == (1 if out["end_flags"][c] & GM.BLACK_KING_GONE else -1)


def test_the_first_ply_that_is_not_king_safe():
    moves, lens, results, rows, g = GM.golden_games()
    out = GM.replay(None, None, moves, lens, results, 1)
    first = [int(v) if s != GM.OK else None for v, s in zip(out["valid"], out["status"])]
    assert first == [33, 49, 46, None, 9, 6]
    # game 0 is mated at ply 33 (no king-safe move at all: the reference plays on until the king falls); the others leave a king attacked
    assert [int(s) for s in out["status"]] == [GM.AFTER_END, GM.ILLEGAL, GM.ILLEGAL, GM.OK, GM.ILLEGAL, GM.ILLEGAL]
    assert out["end_flags"][0] & 4 and out["end_flags"][0] & 1
    # the plies given but not made are zero records, the plies made carry lists that are subsets of the reference's
    at = 0
    for c in range(6):
        recs = out["records"][at:at + lens[c]]
        assert (recs[out["valid"][c]:] == 0).all() and (recs[:out["valid"][c], 91] <= g["count"][rows[c]][:out["valid"][c]]).all()
        at += lens[c]


def test_the_fault_corpus_is_what_it_says():
    import games_cases as GC
    c = GC.corpus()   # asserts its own coverage
    assert c["moves"].shape == (130, 48) and len(c["notes"]) >= 12
