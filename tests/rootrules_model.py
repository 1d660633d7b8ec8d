"""Host model of the root rules shared by the match and self-play (csrc/cz_rootrules.h) — TEST INFRASTRUCTURE: the rule level
of a game, the history of its root positions with the verdict on each, and the king-safe root children.  Everything the game
loops of tests/match_model.py and tests/selfplay_rules_model.py do in front of the choice is here."""
import chase_model as CM
import kingsafe_model as KM
import repetition_model as RM

CAPTURE, KINGSAFE, REPETITION, CHASE = 0, 1, 2, 3        # CZ_RULES_*: each level includes the ones below it


def level(rules, fold, chase):
    """cz_rules_level: rules "xiangqi" (or 1), else the reference's king-capture game."""
    if rules not in ("xiangqi", 1):
        return CAPTURE
    return KINGSAFE if not fold else (CHASE if chase else REPETITION)


class History:
    """wave_root_history: the keys and check flags of a game's root positions — with their chase records at the chase level, or
    when records is set — and the verdict of the rule on each new one.  preset {i: key}: a hand-set ring — the key of position i
    is overwritten once the verdict on position i is in, as a test overwrites ring_key[i & 63] between two chooses; the rule
    reads the ring, not the game, so this is the one way to a verdict on a position that is mate (its first occurrence ends
    a game)."""

    def __init__(self, level, fold, records=False, preset=None):
        self.level, self.fold, self.keep = level, fold, records or level >= CHASE
        self.keys, self.checks, self.records = [], [], []
        self.preset = dict(preset or {})

    def root(self, board, side, rr, ply):
        """Append the root (board, side to move) of ply `ply` -> (code, first, cause) with window min(rr, ply, 63); the cause is
        CAUSE_NONE below the chase level."""
        from oracle import oracle as O
        self.keys.append(int(O.zhash(board, side)))
        self.checks.append(1 if KM.attacked(board, side) else 0)
        if self.keep:
            self.records.append(CM.record(board, side))
        window = min(int(rr), ply, 63)
        out = RM.NONE, -1, CM.CAUSE_NONE
        if self.level >= CHASE:
            out = CM.verdict(self.keys, self.checks, self.records, side, window, self.fold)
        elif self.level >= REPETITION:
            out = RM.verdict(self.keys, self.checks, side, window, self.fold) + (CM.CAUSE_NONE,)
        if ply in self.preset:
            self.keys[ply] = int(self.preset[ply])
        return out


def safe_children(board, side, labels):
    """Indices, in generation order, of the root children whose move is king-safe on (board, side)."""
    safe = set(int(x) for x in KM.kingsafe(board, side)[0])
    return [i for i, l in enumerate(labels) if int(l) in safe]
