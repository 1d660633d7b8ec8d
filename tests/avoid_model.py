"""Host model of the avoid step of matches and self-play (cz_match_set_avoid / cz_selfplay_set_avoid) — TEST INFRASTRUCTURE.  The
game loops of tests/match_model.py and tests/selfplay_rules_model.py ask rootrules_model for the history's verdict and then for
the king-safe root children; avoiding() makes them run with the avoid step in between, without a second game loop: the king-safe
children lose the moves that tests/repmoves_model.py calls losing on the history the loop has just extended (the window the
rule's own, min(rr, ply, 63), no window past 63), unless every move loses."""
import contextlib

import repmoves_model as M
import rootrules_model as RR


@contextlib.contextmanager
def avoiding(counters=None):
    """Inside: every RR.History made remembers the root it was last asked about, and RR.safe_children filters by it.  counters
    (a dict): gains avoided / forced_repetitions, counted at the plies at which the king-safe children are asked for."""
    counters = {} if counters is None else counters
    counters.setdefault("avoided", 0)
    counters.setdefault("forced_repetitions", 0)
    base_history, base_safe = RR.History, RR.safe_children
    last = {}

    class History(base_history):
        def root(self, board, side, rr, ply):
            out = super().root(board, side, rr, ply)
            last["h"], last["at"] = self, (bytes(bytearray(board)), int(side), int(rr), int(ply))
            return out

    def safe_children(board, side, labels):
        idx = base_safe(board, side, labels)
        h = last.get("h")
        if h is None or h.level < RR.REPETITION or not idx:
            return idx
        _, s, rr, ply = last["at"]
        assert last["at"][0] == bytes(bytearray(board)) and s == side and len(h.keys) == ply + 1
        res = M.repetition_moves(board, side, h.keys, h.checks, h.records if h.level >= RR.CHASE else None, min(rr, ply, 63), h.fold, wcap=63)
        counters["avoided"] += 1 if res["summary"] & M.REMOVED else 0
        counters["forced_repetitions"] += 1 if res["summary"] & M.FORCED else 0
        allowed = set(res["allowed"])
        return [i for i in idx if int(labels[i]) in allowed]

    RR.History, RR.safe_children = History, safe_children
    try:
        yield counters
    finally:
        RR.History, RR.safe_children = base_history, base_safe
