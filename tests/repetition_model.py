"""The model of the repetition rule (TEST INFRASTRUCTURE): include/cchess_hip.h cz_repetition in plain Python.

A history is the sequence of a game's positions, position 0 the opening: keys[i] identifies position i (board and side to
move), in_check[i] says that the side to move at i is attacked.  cz_repetition and the match's choose kernel are held to this
file bit for bit."""
NONE, DRAW, RED_LOSES, BLACK_LOSES = 0, 1, 2, 3


def verdict(keys, in_check, side_now, window=None, fold=3):
    """keys / in_check: positions 0 .. n, the last one current, side_now to move in it (0 red, 1 black); window: how many
    earlier positions count (None: all; clamped to 0 .. n) -> (code, first): first = j, the (fold - 1)-th most recent
    earlier occurrence of the current position, or -1."""
    n = len(keys) - 1
    w = n if window is None else max(0, min(int(window), n))
    occ = [i for i in range(n - 1, n - w - 1, -1) if keys[i] == keys[n]]      # most recent first
    if len(occ) < fold - 1:
        return NONE, -1
    j = occ[fold - 2]
    cycle = range(j + 1, n + 1)
    side = lambda i: (side_now ^ (n - i)) & 1                                  # the side to move at position i
    perpetual = []
    for x in (0, 1):                                                           # x checked with every one of its moves in the cycle
        reached = [i for i in cycle if side(i) == 1 - x]
        perpetual.append(len(reached) > 0 and all(bool(in_check[i]) for i in reached))
    if perpetual[0] == perpetual[1]:
        return DRAW, j
    return (RED_LOSES if perpetual[0] else BLACK_LOSES), j
