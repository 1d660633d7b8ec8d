"""Inputs of the record-expansion tests (test_records_cpu.py, test_hip_records.py): the 342 plies of tests/golden/selfplay.npz as
packed records, and constructed records at the edges of the format."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def file_mirror(label):
    """'a0b2' -> 'i0h2': both files mirrored across the e-file, ranks unchanged"""
    return "".join("ihgfedcba"["abcdefghi".index(c)] if c.isalpha() else c for c in label)


def golden():
    """-> (records u8 [342, 608], pi f64 [342, 2086]: the reference's own dense pi in canonical orientation)"""
    from cchess_zero_amd.selfplay import canonical_boards, pack_records
    g = np.load(os.path.join(ROOT, "tests", "golden", "selfplay.npz"))
    n = len(g["side"])
    pi = np.zeros((n, 2086), np.float64)
    for r in range(n):
        lo, hi = int(g["pi_ptr"][r]), int(g["pi_ptr"][r + 1])
        pi[r, g["pi_idx"][lo:hi]] = g["pi_val"][lo:hi]
    boards = canonical_boards(g["state"], g["side"])   # try_flip is an involution: the real board of a canonical state
    labels = np.where(np.arange(128)[None, :] < g["count"][:, None], g["labels"], 0xFFFF).astype(np.uint16)
    rec = pack_records(boards, g["side"], labels, g["visits"], g["count"], g["z"].astype(np.int8), ply=np.arange(n) % 400)
    return rec, pi


def constructed():
    """Records at the edges: counts 0, 1, 64, 65 and 128; visits with zeros among them, no visit at all, a saturated 65535; both
    movers; the start position (its own mirror image) and game positions; a child on a fixed-point label of the mirror (an
    e-file vertical move) in every record that has children.  Labels are distinct within a record."""
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.rules import START_BOARD
    from cchess_zero_amd.selfplay import pack_records
    t = tables()
    rng = np.random.default_rng(20260925)
    g = np.load(os.path.join(ROOT, "tests", "golden", "rules.npz"))
    fixed = [t["label2i"][s] for s in ("e0e1", "e9e8", "e3e4", "e6e5")]
    boards, side, labels, visits, counts, z = [], [], [], [], [], []
    kinds = ("plain", "zeros", "none", "saturated")
    for ci, count in enumerate((0, 1, 64, 65, 128)):
        for ki, kind in enumerate(kinds):
            for mover in (0, 1):
                j = len(boards)
                boards.append(START_BOARD if (ci + ki + mover) % 3 == 0 else g["boards"][(97 * j + 11) % len(g["boards"])])
                side.append(mover)
                lab = np.full(128, 0xFFFF, np.uint16)
                vis = np.zeros(128, np.int64)
                if count:
                    f = fixed[j % len(fixed)]
                    others = rng.permutation(np.setdiff1d(np.arange(2086), [f]))[:count - 1]
                    lab[:count] = rng.permutation(np.concatenate([[f], others]))
                    if kind != "none":
                        vis[:count] = rng.integers(1, 400, count)
                        if kind == "zeros":
                            vis[:count][rng.random(count) < 0.5] = 0
                            vis[rng.integers(count)] = 7        # at least one visit stays
                        if kind == "saturated":
                            vis[rng.integers(count)] = 70000    # pack_records stores 65535 and sets the flag
                labels.append(lab)
                visits.append(vis)
                counts.append(count)
                z.append((-1, 0, 1)[j % 3])
    return pack_records(np.array(boards, np.uint8), np.array(side, np.uint8), np.array(labels), np.array(visits), np.array(counts, np.uint8),
                        np.array(z, np.int8), ply=np.arange(len(z)))


def all_records():
    return np.concatenate([golden()[0], constructed()])
