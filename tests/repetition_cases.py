"""Shared inputs of the repetition tests (TEST INFRASTRUCTURE): the constructed perpetual check and the CPU-made openings."""
import numpy as np

import fakenet

PERPETUAL_PLAYOUTS = 30
PERPETUAL_LINE = ["e5d5", "d9e9", "d5e5", "e9d9"]


def perpetual_board():
    """Red king f0, red rook e5, black king d9, red to move: Rd5+ Ke9, Re5+ Kd9 and the position is back."""
    b = np.zeros(90, np.uint8)
    b[5], b[49], b[84] = 1, 3, 8
    return b


def perpetual_checked_positions():
    """The two checked positions of the line (black to move): after Rd5+ and after Re5+."""
    after_rd5 = np.zeros(90, np.uint8)
    after_rd5[5], after_rd5[48], after_rd5[84] = 1, 3, 8
    after_re5 = np.zeros(90, np.uint8)
    after_re5[5], after_re5[49], after_re5[85] = 1, 3, 8
    return [after_rd5, after_re5]


def steering_forward():
    """logits all 1; value -0.9 on the two checked positions of the line (the checked side sees a lost position, so the
    checking side's search prefers the checks), +0.5 elsewhere.  A numpy forward on planes [B, 9, 10, 14]."""
    from oracle import oracle as O
    keys = np.array([fakenet.position_key(O.encode_planes(b, 1)[None])[0] for b in perpetual_checked_positions()], np.uint64)

    def forward(planes):
        planes = np.asarray(planes, np.float32)
        if planes.ndim == 3:
            planes = planes[None]
        hit = np.isin(fakenet.position_key(planes), keys)
        return np.ones((planes.shape[0], 2086), np.float32), np.where(hit, np.float32(-0.9), np.float32(0.5)).astype(np.float32).reshape(-1, 1)
    return forward


def steering_device_forward():
    """steering_forward for the HIP engine, as match_model.device_forward wraps fakenet."""
    import torch
    f = steering_forward()

    def forward(planes):
        lg, v = f(planes.float().cpu().numpy())
        return torch.from_numpy(lg).to(planes.device), torch.from_numpy(v).to(planes.device)
    return forward


def cpu_openings(n=8, plies=4, seed=11):
    """The first n positions, distinct by zhash and with both kings, after `plies` uniform random pseudo-legal plies from the
    start position, made with the CPU oracle -> (boards [n, 90], side [n])."""
    from oracle import oracle as O
    rng = np.random.default_rng(seed)
    seen, boards, side = set(), [], []
    while len(boards) < n:
        b, s = O.fen_to_board(O.START_FEN), 0
        for _ in range(plies):
            mv = O.legal_moves(b, s)
            b = O.apply_move(b, int(mv[rng.integers(len(mv))]))[0]
            s ^= 1
        k = O.zhash(b, s)
        if k in seen or not (b == 1).any() or not (b == 8).any():
            continue
        seen.add(k)
        boards.append(b); side.append(s)
    return np.stack(boards), np.array(side, np.uint8)
