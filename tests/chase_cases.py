"""Constructed positions and game lines for the perpetual-chase rule (TEST INFRASTRUCTURE): the table of expected threatened
sets and the four-move chase line, shared by the CPU and the GPU tests."""
import numpy as np

import chase_model as CM
import fakenet
from oracle import oracle as O

CODE = {c: i + 1 for i, c in enumerate("KARBNPC")}
CODE.update({c.lower(): v + 7 for c, v in list(CODE.items())})


def sq(name):
    return 9 * int(name[1]) + "abcdefghi".index(name[0])


def board(pieces, kings=("Kd0", "ke9")):
    """pieces: strings like 'Ra6' (upper case red) -> [90] uint8"""
    b = np.zeros(90, np.uint8)
    for p in tuple(kings) + tuple(pieces):
        assert b[sq(p[1:])] == 0, p
        b[sq(p[1:])] = CODE[p[0]]
    return b


# (name, board, side to move, expected threatened squares)
TABLE = [
    ("rook on a cannon", board(["Ra6", "cb6"]), 1, [55]),
    ("the cannon protected by a rook", board(["Ra6", "cb6", "rb9"]), 1, []),
    ("knight on a protected rook", board(["Nc4", "rb6", "rb9"]), 1, [55]),
    ("knight with a pawn on its leg", board(["Nc4", "cb6", "Pc5"]), 1, []),
    ("pinned rook, black to move", board(["Re3", "re8", "ca3"], kings=("Ke0", "kd9")), 1, []),
    ("pinned rook, red to move", board(["Re3", "re8", "ca3"], kings=("Ke0", "kd9")), 0, []),
    ("uncrossed pawn", board(["Ra4", "pa6"]), 1, []),
    ("crossed pawn", board(["Ra2", "pa4"]), 1, [36]),
    ("pawn attacker", board(["Pe6", "ne7"]), 1, []),
    ("cannon over a screen", board(["Ca0", "Pa3", "na6"]), 1, [54]),
    ("the king on e9 protects e8", board(["Ra8", "ce8"]), 1, []),
    ("no flying general onto e5", board(["Ra5", "ce5"]), 1, [49]),
]

# the constructed chase: the rook follows the cannon up and down, played twice; red moves first
CHASE_BOARD = board(["Ra5", "cb6"])
CHASE_LINE = ["a5a6", "b6b5", "a6a5", "b5b6"] * 2
CHASE_THREATS = [[], [55], [], [46]] * 2 + [[]]
CHASE_PLAYOUTS = 30          # of a search that steering_forward leads along the line


def label_of(move, lut=None):
    lut = O.lut() if lut is None else lut
    return int(lut[sq(move[:2]), sq(move[2:])])


def play_line(start, side, moves, mirrored=False):
    """-> (boards [n + 1, 90], sides [n + 1], labels [n]): the positions of the line; mirrored: the same game with the colours
    swapped (the start board mirrored, every move mirrored, the other side first)"""
    lut = O.lut()
    b, s = (CM.mirror(start), 1 - side) if mirrored else (np.array(start, np.uint8), side)
    boards, sides, labels = [b.copy()], [s], []
    for m in moves:
        a, t = sq(m[:2]), sq(m[2:])
        if mirrored:
            a, t = CM.mirror_sq(a), CM.mirror_sq(t)
        l = int(lut[a, t])
        assert l >= 0 and l in O.legal_moves(b, s).tolist(), m
        b = O.apply_move(b, l)[0]
        s ^= 1
        boards.append(b.copy()); sides.append(s); labels.append(l)
    return np.stack(boards), np.array(sides, np.uint8), labels


def history(boards, sides):
    """-> (keys uint64 [n], in_check uint8 [n], records uint64 [n, 4]) of a line's positions"""
    from kingsafe_model import attacked
    keys = np.array([O.zhash(b, int(s)) for b, s in zip(boards, sides)], np.uint64)
    chk = np.array([attacked(b, int(s)) for b, s in zip(boards, sides)], np.uint8)
    return keys, chk, CM.records(boards, sides)


def synthetic_cycle(threat_even, threat_odd, check_even=0, check_odd=0, plies=8):
    """A history of plies + 1 positions that repeats with period 4 and in which the side to move shuffles one piece between
    squares 0 and 1 (even positions) / 80 and 81 (odd positions) while its piece on 40 / 50 stands: threat_even / threat_odd
    say whether that standing piece is threatened in the even / odd positions -> (keys, in_check, records) as lists."""
    keys, chk, recs = [], [], []
    for i in range(plies + 1):
        keys.append(1000 + i % 4)
        odd = i & 1
        mover = (80 if odd else 0) + ((i >> 1) & 1)
        stand = 50 if odd else 40
        own = (1 << mover) | (1 << stand)
        t = (1 << stand) if (threat_odd if odd else threat_even) else 0
        chk.append(check_odd if odd else check_even)
        recs.append([t & CM.MASK64, t >> 64, own & CM.MASK64, own >> 64])
    return keys, chk, recs


def steering_forward():
    """A numpy forward on planes [B, 9, 10, 14] that makes a search play CHASE_LINE.  The reference's root never counts its
    own visits, so at the root U = 0 and the choice among the root children is by Q alone: a policy cannot steer it, the values
    do.  Value 0 on the four positions of the line (keyed by fakenet.position_key of their planes), +0.9 for the side to move
    everywhere else: whoever leaves the line hands the other side a good position, so the line's move is every root's only child
    with Q >= 0 and takes the visits left once each child has been tried.  Logits all 1."""
    boards, sides, _ = play_line(CHASE_BOARD, 0, CHASE_LINE[:4])
    keys = np.array([fakenet.position_key(O.encode_planes(boards[i], int(sides[i]))[None])[0] for i in range(4)], np.uint64)

    def forward(planes):
        planes = np.asarray(planes, np.float32)
        if planes.ndim == 3:
            planes = planes[None]
        hit = np.isin(fakenet.position_key(planes), keys)
        return np.ones((planes.shape[0], 2086), np.float32), np.where(hit, np.float32(0.0), np.float32(0.9)).astype(np.float32).reshape(-1, 1)
    return forward


def steering_device_forward():
    import torch
    f = steering_forward()

    def forward(planes):
        lg, v = f(planes.float().cpu().numpy())
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    return forward
