"""Host-side verifier of the evaluation caches' entries (cz_search_set_eval_cache / cz_search_set_xcache) against the C oracle.

A cache entry stands for one evaluated position: its packed board, its key, its legal moves in generation order with their
(src, dst), the priors the expansion gave them and the value it backed up.  A hit expands a leaf from the entry without asking
the net, so every one of these must be what the oracle computes for the stored position — an entry whose parts come from two
different positions hands a tree moves that are not legal in it.  The checks here read the tables back
(SearchEngine.xcache_dump / eval_cache_dump) and compare every non-empty entry with the oracle, exactly (bit for bit for the
floats).  `expand` callbacks give the reference priors and value: `oracle_expander(fwd)` for the fake net, or a second engine
for the real one.
"""
import numpy as np

from oracle import oracle as O

BUSY = 1 << 63                   # reserved key bit: a cross-tree entry being written, key | BUSY (cz_evalcache.h: CZ_XC_BUSY)
FULL_MASK = 0xFFFFFFFFFFFFFFFF
EC_BUCKETS = 128


def key_mask(bits):
    """The key mask cz_search_debug_eval_cache_key_bits(bits) sets."""
    return FULL_MASK if bits == 64 else ((0x7F << 17) | ((1 << (bits - 7)) - 1))


def position_key(board, side, mask=FULL_MASK):
    """The cache key of a position, as the select kernels compute it: the Zobrist key (cz_hash) without the reserved BUSY bit,
    0 -> 1, masked, and 0 -> 1 again."""
    h = (O.zhash(board, side) & ~BUSY) or 1
    h &= mask
    return h or 1


def pack_board(board, side):
    """wave_pack_board: 90 squares x 4 bits in 12 dwords (square 8j + k in nibble k of word j), side in the top nibble of word 11."""
    b = np.zeros(96, np.uint32)
    b[:90] = np.asarray(board, np.uint8)
    w = np.zeros(12, np.uint32)
    for k in range(8):
        w |= b[k::8] << np.uint32(4 * k)
    w[11] |= np.uint32(int(side) << 28)
    return w


def unpack_board(words):
    """The inverse of pack_board -> (board uint8 [90], side, list of problems)."""
    words = np.asarray(words, np.uint32)
    nib = np.stack([(words >> np.uint32(4 * k)) & np.uint32(15) for k in range(8)], axis=1).reshape(96).astype(np.uint8)
    board, side = nib[:90].copy(), int(nib[95])
    bad = []
    if nib[90:95].any():
        bad.append("nonzero padding nibbles %s" % nib[90:95].tolist())
    if (board > 14).any():
        bad.append("piece code 15")
    if int((board == 1).sum()) != 1 or int((board == 8).sum()) != 1:
        bad.append("kings: %d red, %d black" % (int((board == 1).sum()), int((board == 8).sum())))
    if side not in (0, 1):
        bad.append("side to move %d" % side)
    return board, side, bad


def oracle_expander(fwd, cap=256):
    """-> expand(positions): the oracle's expansion of each (board, side) as the root of a fresh tree, fed by the fake net
    `fwd`: per position (priors f32 [count] of the root's children, value f32 = -v as k_expand_backup backs it up)."""
    def expand(positions):
        if not positions:
            return []
        S = O.Search(len(positions), cap)
        S.reset(np.stack([p[0] for p in positions]), np.array([p[1] for p in positions], np.uint8),
                np.zeros(len(positions), np.int32))
        planes, need = S.select(0)
        assert need.all()
        lg, v = fwd(planes)
        S.expand_backup(lg, v)
        rs = S.root_stats()
        vv = (np.asarray(v, np.float32).reshape(-1) * np.float32(-1.0)).astype(np.float32)
        return [(rs["P"][i, :int(rs["count"][i])].copy(), np.float32(vv[i])) for i in range(len(positions))]
    return expand


class Reference:
    """Memoised per-position reference: legal labels in order, their (src, dst), priors and value."""

    def __init__(self, expand):
        self.expand = expand
        self.memo = {}
        self.srcdst = O.label_srcdst()

    def get(self, positions):
        todo, seen = [], set()
        for b, s in positions:
            k = (np.asarray(b, np.uint8).tobytes(), int(s))
            if k not in self.memo and k not in seen:
                seen.add(k)
                todo.append((np.asarray(b, np.uint8), int(s)))
        for (b, s), (P, v) in zip(todo, self.expand(todo)):
            lab = O.legal_moves(b, s)
            assert len(P) == len(lab), "the reference expansion has %d priors for %d legal moves" % (len(P), len(lab))
            self.memo[(b.tobytes(), s)] = (lab, self.srcdst[lab], np.asarray(P, np.float32), np.float32(v))
        return [self.memo[(np.asarray(b, np.uint8).tobytes(), int(s))] for b, s in positions]


def _fail(problems, what):
    if problems:
        raise AssertionError("%s: %d bad entries, first: %s" % (what, len(problems), "; ".join(problems[:8])))


def check_xcache(dump, ref, mask=FULL_MASK, max_ply=0xFFFF, check_values=True):
    """Every non-empty entry of a cross-tree table dump (SearchEngine.xcache_dump) against the oracle.  ref: Reference.
    check_values=False leaves priors and value out (structure only).  Raises AssertionError listing the bad entries;
    returns dict(entries, duplicates = entries holding a position another entry holds too, distinct positions)."""
    key = dump["key"]
    n = len(key)
    xc_mask = n // 64 - 1
    bad, live, pos = [], [], []
    for e in np.nonzero(key)[0]:
        k = int(key[e])
        if k & BUSY:
            bad.append("entry %d: key %016x still carries the reserved BUSY bit (a claim never published)" % (e, k))
            continue
        board, side, why = unpack_board(dump["board"][e])
        if why:
            bad.append("entry %d: board %s" % (e, ", ".join(why)))
            continue
        if k != position_key(board, side, mask):
            bad.append("entry %d: key %016x, the position's is %016x" % (e, k, position_key(board, side, mask)))
        if ((k >> 24) & xc_mask) != e // 64:
            bad.append("entry %d: key %016x belongs to bucket %d, not %d" % (e, k, (k >> 24) & xc_mask, e // 64))
        if int(dump["ply"][e]) > max_ply:
            bad.append("entry %d: ply %d > %d" % (e, int(dump["ply"][e]), max_ply))
        live.append(e)
        pos.append((board, side))
    refs = ref.get(pos)
    for e, (lab, sd, P, v) in zip(live, refs):
        c = int(dump["count"][e])
        if c != len(lab):
            bad.append("entry %d: count %d, the position has %d legal moves" % (e, c, len(lab)))
            continue
        if not np.array_equal(dump["label"][e, :c], lab):
            bad.append("entry %d: labels differ from the ordered legal list at %s" % (e, np.nonzero(dump["label"][e, :c] != lab)[0][:6].tolist()))
        if not np.array_equal(dump["sd"][e, :c], sd):
            bad.append("entry %d: (src, dst) differ from the labels' at %s" % (e, np.nonzero(dump["sd"][e, :c] != sd)[0][:6].tolist()))
        if check_values:
            if not np.array_equal(dump["P"][e, :c].view(np.uint32), P.view(np.uint32)):
                bad.append("entry %d: priors differ at %s" % (e, np.nonzero(dump["P"][e, :c].view(np.uint32) != P.view(np.uint32))[0][:6].tolist()))
            if np.float32(dump["value"][e]).view(np.uint32) != np.float32(v).view(np.uint32):
                bad.append("entry %d: value %r, the expansion backs up %r" % (e, float(dump["value"][e]), float(v)))
    _fail(bad, "cross-tree cache")
    distinct = len({dump["board"][e].tobytes() for e in live})
    return dict(entries=len(live), duplicates=len(live) - distinct, distinct=distinct)


def _record_parents(tree):
    """Parent record of every pre-order record of a tree dump (-1: a child of the root)."""
    par = np.full(len(tree), -1, np.int64)
    stack = []
    for r, d in enumerate(tree[:, 0].tolist()):
        del stack[d:]
        par[r] = stack[-1] if stack else -1
        stack.append(r)
    return par


def _children(tree, r):
    """Records of the children of record r (-1: of the root), in order."""
    d = 0 if r < 0 else int(tree[r, 0]) + 1
    out, i = [], r + 1
    while i < len(tree) and tree[i, 0] >= d:
        if tree[i, 0] == d:
            out.append(i)
        i += 1
    return out


def check_eval_cache(ec, tree, root_board, root_side, ref, mask=FULL_MASK):
    """Every non-empty per-tree entry of tree g (SearchEngine.eval_cache_dump(g)) against its tree (tree_dump(g)) and the oracle:
    the node is in the tree and expanded; the position reached by applying the labels from the root packs to the stored board;
    the key is that position's (and lies in its bucket); the node's children are the ordered legal list with the reference's
    priors; the value is what the reference's expansion backs up.  Returns the number of entries checked."""
    par = _record_parents(tree)
    bad, live, pos = [], [], []
    for i in np.nonzero(ec["key"])[0]:
        r = int(ec["record"][i])
        if r == -2:
            bad.append("entry %d: node %d is not in the tree" % (i, int(ec["node"][i])))
            continue
        if r >= 0 and tree[r, 6] < 0:
            bad.append("entry %d: node %d (record %d) is not expanded" % (i, int(ec["node"][i]), r))
            continue
        path, q = [], r
        while q >= 0:
            path.append(int(tree[q, 1]))
            q = int(par[q])
        b = np.asarray(root_board, np.uint8).copy()
        for lab in reversed(path):
            b = O.apply_move(b, lab)[0]
        side = int(root_side) ^ (len(path) & 1)
        k = int(ec["key"][i])
        if not np.array_equal(ec["board"][i], pack_board(b, side)):
            bad.append("entry %d: stored board is not the position of node %d (record %d)" % (i, int(ec["node"][i]), r))
        if k != position_key(b, side, mask):
            bad.append("entry %d: key %016x, the node's position has %016x" % (i, k, position_key(b, side, mask)))
        if ((k >> 17) & (EC_BUCKETS - 1)) != i // 64:
            bad.append("entry %d: key %016x belongs to bucket %d" % (i, k, (k >> 17) & (EC_BUCKETS - 1)))
        live.append((i, r))
        pos.append((b, side))
    for (i, r), (lab, _sd, P, v) in zip(live, ref.get(pos)):
        ch = _children(tree, r)
        got = tree[ch, 1].astype(np.uint16)
        if len(ch) != len(lab) or not np.array_equal(got, lab):
            bad.append("entry %d: the node's %d children are not its position's %d ordered legal moves" % (i, len(ch), len(lab)))
        elif not np.array_equal(tree[ch, 5].astype(np.int32).view(np.uint32), P.view(np.uint32)):
            bad.append("entry %d: the node's children's priors are not the reference expansion's" % i)
        if np.float32(ec["value"][i]).view(np.uint32) != np.float32(v).view(np.uint32):
            bad.append("entry %d: value %r, the expansion backs up %r" % (i, float(ec["value"][i]), float(v)))
    _fail(bad, "per-tree cache")
    return len(live)
