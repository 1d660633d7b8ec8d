"""tests/repmoves_model.py — the two-ply repetition verdicts on root moves that cz_repetition_moves is held to — on the constructed
lines, on made-up records, and against the live rule of the game loops (rootrules_model.History) over random walks.  No GPU."""
import numpy as np

import chase_cases as CC
import chase_model as CM
import kingsafe_model as KM
import repetition_cases as RC
import repmoves_model as M
import rootrules_model as RR
from oracle import oracle as O

LABEL = {s: i for i, s in enumerate(O.labels())}
RED_BY_CHECK = M.RED_LOSES | (CM.CAUSE_CHECK << 4)
RED_BY_CHASE = M.RED_LOSES | (CM.CAUSE_CHASE << 4)


def named(prefix, fold, kind, position):
    name = "%s fold %d %s position %d" % (prefix, fold, kind, position)
    return [c for c in M.constructed_cases() if c["name"] == name][0]


def of(res, move):
    j = res["moves"].index(LABEL[move])
    return res["verdict"][j], res["reply"][j], res["reply_verdict"][j], LABEL[move] in res["allowed"]


def test_constructed_perpetual_check():
    for kind in ("check", "chase"):
        # fold 3: red's last chance is position 6 — d5e5 repeats nothing, black's answer e9d9 ends the game
        r = M.model_of(named("perpetual", 3, kind, 6))
        assert of(r, "d5e5") == (M.NONE, LABEL["e9d9"], RED_BY_CHECK, False) and r["summary"] == M.REMOVED
        assert len(r["allowed"]) == len(r["moves"]) - 1
        r = M.model_of(named("perpetual", 3, kind, 7))
        assert of(r, "e9d9") == (RED_BY_CHECK, M.NO_REPLY, 0, True) and r["summary"] == M.OPP_LOSES
        # fold 2: the same one cycle — two moves of each side — earlier
        r = M.model_of(named("perpetual", 2, kind, 2))
        assert of(r, "d5e5") == (M.NONE, LABEL["e9d9"], RED_BY_CHECK, False) and r["summary"] == M.REMOVED
        r = M.model_of(named("perpetual", 2, kind, 3))
        assert of(r, "e9d9") == (RED_BY_CHECK, M.NO_REPLY, 0, True) and r["summary"] == M.OPP_LOSES
        # fold 4: nothing up to position 9
        for i in range(10):
            r = M.model_of(named("perpetual", 4, kind, i))
            assert r["summary"] == 0 and not any(r["verdict"]) and not any(r["reply_verdict"]) and r["allowed"] == r["moves"]
        for i in range(6):
            assert M.model_of(named("perpetual", 3, kind, i))["summary"] == 0


def test_constructed_chase():
    r = M.model_of(named("chase", 3, "chase", 6))
    assert of(r, "a6a5") == (M.NONE, LABEL["b5b6"], RED_BY_CHASE, False) and r["summary"] == M.REMOVED
    r = M.model_of(named("chase", 3, "chase", 7))
    assert of(r, "b5b6") == (RED_BY_CHASE, M.NO_REPLY, 0, True) and r["summary"] == M.OPP_LOSES
    # the record from position 1 on: the chaser's own a5a6 completes the third occurrence
    r = M.model_of(named("chase, the chaser completes", 3, "chase", 7))
    assert of(r, "a5a6")[0] == RED_BY_CHASE and not of(r, "a5a6")[3] and r["summary"] == M.REMOVED
    # without the chase records the same repetition is a draw, and a draw stays allowed
    r = M.model_of(named("chase, the chaser completes", 3, "check", 7))
    assert of(r, "a5a6") == (M.DRAW, M.NO_REPLY, 0, True) and r["summary"] == 0


def test_capture_cut_window_and_quiet_shuffle():
    cases, take, quiet = M.made_up_cases()
    res = {c["name"]: M.model_of(c) for c in cases}
    for name, r in res.items():
        j = r["moves"].index(take if name.startswith("capture") else quiet)
        want = M.DRAW if name in ("quiet", "quiet window 2") else M.NONE       # window 2 -> 3 reaches the occurrence two plies back
        assert r["verdict"][j] == want, name
        assert sum(1 for v in r["verdict"] if v) == (1 if want else 0) and r["summary"] == 0 and r["allowed"] == r["moves"], name


def test_forced_and_wide():
    r = M.model_of(M.forced_case())
    assert len(r["moves"]) == 1 and r["verdict"] == [RED_BY_CHECK] and r["allowed"] == r["moves"] and r["summary"] == M.FORCED
    c, j = M.wide_case()
    r = M.model_of(c)
    assert len(r["moves"]) > 64 and j >= 64 and r["losing"][j] and r["summary"] & M.REMOVED and r["moves"][j] not in r["allowed"]
    assert set(r["allowed"]) | {m for m, l in zip(r["moves"], r["losing"]) if l} == set(r["moves"])


def test_random_walks_agree_with_the_live_rule_and_find_every_kind():
    """For every prefix of every walk the own verdict of the move actually played is History.root's verdict on the next
    position, and the verdict of the reply actually played is the one on the position after that whenever the game got there
    (no verdict in between) and the reply is the first losing one; the counts say that the corpus holds every kind."""
    cases = M.walk_reference()
    by_game = {}
    for c in cases:
        by_game.setdefault(c["game"], []).append(c)
    checked = replies = 0
    for g, cs in by_game.items():
        h = RR.History(RR.CHASE, M.WALK_FOLD)
        boards = [c["board"] for c in cs]
        live = [h.root(c["board"], c["side"], c["window"], c["ply"]) for c in cs]     # rr = plies since a capture, as windows_of
        assert [c["ply"] for c in cs] == list(range(len(cs))) and all(c["window"] <= c["ply"] for c in cs)
        for i, c in enumerate(cs[:-1]):
            r = c["res"]
            j = r["moves"].index(c["played"])
            code, _, cause = live[i + 1]
            assert r["verdict"][j] == code | (cause << 4), (g, i)
            checked += 1
            if i + 2 < len(cs) and code == M.NONE:
                code2, _, cause2 = live[i + 2]
                loss_m = M.BLACK_LOSES if c["side"] else M.RED_LOSES
                played2 = cs[i + 1]["played"]
                if code2 == loss_m:
                    first = [int(x) for x in KM.kingsafe(boards[i + 1], cs[i + 1]["side"])[0]]
                    assert r["reply_verdict"][j] != 0 and first.index(r["reply"][j]) <= first.index(played2), (g, i)
                    if r["reply"][j] == played2:
                        assert r["reply_verdict"][j] == code2 | (cause2 << 4), (g, i)
                        replies += 1
                elif r["reply"][j] == played2:
                    raise AssertionError((g, i, "the reply played does not lose in the game"))
    counts, some, games = M.walk_counts(cases)
    print("walks: %d games, %d positions, %d with some verdict; %s; %d moves and %d replies checked against the live rule"
          % (games, len(cases), some, counts, checked, replies))
    assert games == M.WALK_GAMES and some * 10 >= games and all(v >= 1 for v in counts.values()), (counts, some, games)
    assert checked >= 400 and replies >= 1
