"""The opening book's model (include/cchess_hip.h: BOOK), independent of the HIP code: canonical keys from the C oracle's Zobrist
hash of the board and of its numpy mirror, labels through tables()["mirror"], entries from packed records by argmax of the
visits, the reduce in plain Python dicts, the probe by np.searchsorted on the unsigned keys, the choice in Python integers."""
import numpy as np

from oracle import oracle as O

REC_BYTES, REC_SIDE, REC_COUNT, REC_Z, REC_PLY, REC_LABELS, REC_VISITS = 608, 90, 91, 92, 94, 96, 352
SKIPPED, NONE = 255, 0xFFFF


def mirror_table():
    from cchess_zero_amd._lib import tables
    return tables()["mirror"].astype(np.int64)


def mirror_board(board):
    return np.ascontiguousarray(np.asarray(board, np.uint8).reshape(10, 9)[:, ::-1]).reshape(90)


def canonical(board, side):
    """-> (key, mirrored 0 / 1 / 2); a byte above 14 counts as an empty square"""
    b = np.asarray(board, np.uint8).copy()
    b[b > 14] = 0
    k, km = O.zhash(b, int(side)) & (2 ** 64 - 1), O.zhash(mirror_board(b), int(side)) & (2 ** 64 - 1)
    return min(k, km), 1 if km < k else 2 if km == k else 0


def canonical_label(label, mirrored):
    m = int(mirror_table()[label])
    return m if mirrored == 1 else min(int(label), m) if mirrored == 2 else int(label)


def own_label(label, mirrored):
    return int(mirror_table()[label]) if mirrored == 1 else int(label)


def keys(boards, side):
    r = [canonical(b, s) for b, s in zip(boards, side)]
    return np.array([x[0] for x in r], np.uint64), np.array([x[1] for x in r], np.uint8)


def entry(rec, max_ply):
    """one packed record -> (key, label, outcome)"""
    rec = np.asarray(rec, np.uint8)
    key, mir = canonical(rec[:90], rec[REC_SIDE])
    count = min(int(rec[REC_COUNT]), 128)
    ply = int(rec[REC_PLY]) | int(rec[REC_PLY + 1]) << 8
    if count == 0 or (max_ply > 0 and ply >= max_ply):
        return key, NONE, SKIPPED
    vis = rec[REC_VISITS:REC_VISITS + 256].view(np.uint16)[:count]
    lab = int(rec[REC_LABELS:REC_LABELS + 256].view(np.uint16)[int(np.argmax(vis))])
    z = int(rec[REC_Z:REC_Z + 1].view(np.int8)[0])
    return key, canonical_label(lab, mir), 0 if z > 0 else 1 if z == 0 else 2


def entries(records, max_ply):
    r = [entry(x, max_ply) for x in records]
    return np.array([x[0] for x in r], np.uint64), np.array([x[1] for x in r], np.uint16), np.array([x[2] for x in r], np.uint8)


def reduce(key, label, outcome):
    """tuples -> the book's arrays (key u64, label u16, games, wins, draws u32), sorted by (key, label)"""
    d = {}
    for k, l, o in zip(key.tolist(), label.tolist(), outcome.tolist()):
        if o == SKIPPED:
            continue
        e = d.setdefault((k, l), [0, 0, 0])
        e[0] += 1
        e[1] += o == 0
        e[2] += o == 1
    pairs = sorted(d)
    return (np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint16),
            np.array([d[p][0] for p in pairs], np.uint32), np.array([d[p][1] for p in pairs], np.uint32), np.array([d[p][2] for p in pairs], np.uint32))


def merge(a, b):
    d = {}
    for t in (a, b):
        for k, l, g, w, dr in zip(*(x.tolist() for x in t)):
            e = d.setdefault((k, l), [0, 0, 0])
            e[0] += g; e[1] += w; e[2] += dr
    pairs = sorted(d)
    return (np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint16),
            np.array([d[p][0] for p in pairs], np.uint32), np.array([d[p][1] for p in pairs], np.uint32), np.array([d[p][2] for p in pairs], np.uint32))


def book_of(records, max_ply):
    return reduce(*entries(records, max_ply))


def probe(bkey, boards, side):
    """-> (first i32, count i32, mirrored u8)"""
    k, mir = keys(boards, side)
    lo, hi = np.searchsorted(bkey, k, "left"), np.searchsorted(bkey, k, "right")
    count = (hi - lo).astype(np.int32)
    return np.where(count > 0, lo, -1).astype(np.int32), count, mir


def choose_one(blabel, bgames, first, count, mirrored, allowed, min_games, mode, rnd):
    """one position -> (played, index); allowed: None, the set of labels (own orientation) or the position's 66 mask words"""
    def ok(l):
        return allowed is None or ((int(allowed[l >> 5]) >> (l & 31)) & 1 if isinstance(allowed, np.ndarray) else l in allowed)
    elig = []
    for i in range(first, first + count):
        own = own_label(int(blabel[i]), mirrored)
        if int(bgames[i]) >= max(min_games, 1) and ok(own):
            elig.append((i, own, int(bgames[i])))
    if not elig:
        return NONE, -1
    if mode == 0:
        best = max(g for _, _, g in elig)
        i, own, _ = [e for e in elig if e[2] == best][0]
        return own, i
    T = sum(g for _, _, g in elig)
    t = (int(rnd) * T) >> 32
    run = 0
    for i, own, g in elig:
        run += g
        if run > t:
            return own, i
    raise AssertionError("t < T")


def choose(book, boards, side, allowed, min_games, mode, rnd, probed=None):
    """allowed: None or [G, 66] uint32 masks; probed: probe()'s answer for these positions, if it is at hand
    -> (played u16 [G], index i32 [G])"""
    first, count, mir = probed or probe(book[0], boards, side)
    played, index = [], []
    for g in range(len(first)):
        al = None if allowed is None else np.asarray(allowed[g], np.uint32)
        p, i = choose_one(book[1], book[2], int(first[g]), int(count[g]), int(mir[g]), al, min_games, mode, 0 if rnd is None else int(rnd[g]))
        played.append(p); index.append(i)
    return np.array(played, np.uint16), np.array(index, np.int32)


# ---- records without a GPU: a game given as ICCS moves from the opening position, by the oracle ---------------------------------
def records_of_game(moves, result):
    """packed records of one game (the legal list is the oracle's pseudo-legal one; visits 1 at the played move)"""
    L = O.labels()
    b, s = O.fen_to_board(O.START_FEN), 0
    out = []
    for ply, m in enumerate(moves):
        l = m if isinstance(m, (int, np.integer)) else L.index(m)
        legal = O.legal_moves(b, s)
        at = int(np.nonzero(legal == l)[0][0])
        rec = np.zeros(REC_BYTES, np.uint8)
        rec[:90], rec[REC_SIDE], rec[REC_COUNT] = b, s, len(legal)
        rec[REC_Z:REC_Z + 1] = np.array([result if s == 0 else -result], np.int8).view(np.uint8)
        rec[REC_PLY:REC_PLY + 2] = np.array([ply], np.uint16).view(np.uint8)
        lab = np.full(128, 0xFFFF, np.uint16)
        lab[:len(legal)] = legal
        vis = np.zeros(128, np.uint16)
        vis[at] = 1
        rec[REC_LABELS:REC_LABELS + 256], rec[REC_VISITS:REC_VISITS + 256] = lab.view(np.uint8), vis.view(np.uint8)
        out.append(rec)
        b, _, _ = O.apply_move(b, l)
        s ^= 1
    return np.stack(out) if out else np.zeros((0, REC_BYTES), np.uint8)


def mirror_moves(moves):
    L, m = O.labels(), mirror_table()
    return [L[int(m[L.index(x)])] for x in moves]
