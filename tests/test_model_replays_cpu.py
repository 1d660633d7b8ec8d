"""The host models of the match and of self-play (tests/match_model.py, tests/selfplay_rules_model.py) against what they computed
when every rule level still had a game loop of its own: tests/golden/model_replays.json was written by those loops, and
tests/golden/gen_model_replays.py rewrites it byte for byte from document() below.  Equality is exact."""
import hashlib
import json
import os

import numpy as np
import pytest

import match_model as MM
from test_selfplay_chase_cpu import whole_games_model

# the 16-game fixture match at every rule level; "chase_off" was the chase loop with its switch off, "repetition" the loop below it
MATCH = dict(capture=dict(rules="capture", fold=0, chase=False), kingsafe=dict(rules="xiangqi", fold=0, chase=False),
             repetition=dict(rules="xiangqi", fold=3, chase=False), chase=dict(), chase_off=dict(chase=False))
# the whole games of tests/test_selfplay_chase_cpu.py; "rules" was the loop without the chase counter
SELFPLAY = dict(chase=dict(), chase_off=dict(chase=False), rules=dict(chase=False))
RULES_STATS = ("games", "red_wins", "black_wins", "draws", "plies", "stalled", "mates", "repetitions", "perpetuals")


def sha256(a, dtype):
    return hashlib.sha256(np.ascontiguousarray(a, dtype).tobytes()).hexdigest()


def match_entry(name, sample_plies):
    m = MM.fakenet_match(sample_plies, **MATCH[name])
    return dict({k: [int(x) for x in m[k]] for k in ("result", "a_red", "plies", "reason")}, moves_sha256=sha256(m["moves"], np.uint16))


def selfplay_entry(name):
    out = whole_games_model(**SELFPLAY[name])
    return dict(stats={k: int(v) for k, v in out["stats"].items() if name != "rules" or k in RULES_STATS},
                outcomes=[[int(t), int(g), o.result, o.how, int(o.fin_n)] for t, g, o in out["outcomes"]],
                records_sha256=sha256(out["records"], np.uint8), picks=int(out["picks"]), unsafe_plies=int(out["unsafe_plies"]),
                min_margin=float(out["min_margin"]).hex(), active=[bool(x) for x in out["active"]])


def document():
    return dict(match={name: {str(sp): match_entry(name, sp) for sp in (0, 6)} for name in MATCH},
                selfplay={name: selfplay_entry(name) for name in SELFPLAY})


@pytest.fixture(scope="module")
def pinned(golden_dir):
    return json.load(open(os.path.join(golden_dir, "model_replays.json")))


@pytest.mark.parametrize("sample_plies", [0, 6])
@pytest.mark.parametrize("name", list(MATCH))
def test_the_fixture_match_is_what_the_separate_loops_replayed(pinned, name, sample_plies):
    assert match_entry(name, sample_plies) == pinned["match"][name][str(sample_plies)]


@pytest.mark.parametrize("name", list(SELFPLAY))
def test_the_whole_selfplay_games_are_what_the_separate_loops_played(pinned, name):
    assert selfplay_entry(name) == pinned["selfplay"][name]


def test_the_levels_nest():
    """Chase off is the repetition game and fold 0 the king-safe game: the same replay, not an equal one."""
    assert MM.fakenet_match(0, chase=False) is MM.fakenet_match(0, "xiangqi", 3, False)
    assert MM.RR.level("xiangqi", 0, True) == MM.RR.KINGSAFE and MM.RR.level("capture", 3, True) == MM.RR.CAPTURE
    assert [MM.RR.level("xiangqi", 3, c) for c in (False, True)] == [MM.RR.REPETITION, MM.RR.CHASE]
