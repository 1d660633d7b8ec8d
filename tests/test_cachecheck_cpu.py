"""The cache verifier (tests/cachecheck.py) is not vacuous: it accepts a correct table built from oracle positions and rejects
every kind of torn or stale entry a racing filing could leave behind.  CPU only (C oracle + fake net)."""
import numpy as np
import pytest

import cachecheck as CC
import fakenet
from conftest import open_boards
from oracle import oracle as O

N_ENTRIES = 128      # two buckets of 64


@pytest.fixture(scope="module")
def table():
    """A correct cross-tree table dump: the start position, its successors (black to move), second-ply positions and open
    boards with more than 64 legal moves (the second half of the 128-slot arrays), each filed in its key's bucket."""
    b0 = O.fen_to_board(O.START_FEN)
    pos = [(b0, 0)]
    for m in O.legal_moves(b0, 0):
        pos.append((O.apply_move(b0, int(m))[0], 1))
    b1 = pos[7][0]
    for m in O.legal_moves(b1, 1)[:10]:
        pos.append((O.apply_move(b1, int(m))[0], 0))
    ob, os_ = open_boards(30, 5)
    long_ = [(ob[i], int(os_[i])) for i in range(len(ob)) if len(O.legal_moves(ob[i], int(os_[i]))) > 64]
    assert len(long_) >= 4
    pos += long_[:8]
    fwd = fakenet.make_forward("signed", 5)
    ref = CC.Reference(CC.oracle_expander(fwd))
    d = dict(key=np.zeros(N_ENTRIES, np.uint64), value=np.zeros(N_ENTRIES, np.float32), count=np.zeros(N_ENTRIES, np.uint16),
             ply=np.zeros(N_ENTRIES, np.uint16), board=np.zeros((N_ENTRIES, 12), np.uint32),
             label=np.zeros((N_ENTRIES, 128), np.uint16), sd=np.zeros((N_ENTRIES, 128), np.uint16),
             P=np.zeros((N_ENTRIES, 128), np.float32))
    fill = [0, 0]
    for (b, s), (lab, sd, P, v) in zip(pos, ref.get(pos)):
        k = CC.position_key(b, s)
        bucket = (k >> 24) & (N_ENTRIES // 64 - 1)
        if fill[bucket] == 64:
            continue
        e = bucket * 64 + fill[bucket]
        fill[bucket] += 1
        n = len(lab)
        d["key"][e], d["value"][e], d["count"][e], d["ply"][e] = k, v, n, 3
        d["board"][e] = CC.pack_board(b, s)
        d["label"][e, :n], d["sd"][e, :n], d["P"][e, :n] = lab, sd, P
    return d, ref


def _entries(d, pred=lambda c: True):
    return [int(e) for e in np.nonzero(d["key"])[0] if pred(int(d["count"][e]))]


def test_board_pack_roundtrip_and_key():
    ob, os_ = open_boards(6, 9)
    for b, s in list(zip(ob, os_)) + [(O.fen_to_board(O.START_FEN), 0)]:
        b2, s2, bad = CC.unpack_board(CC.pack_board(b, s))
        assert not bad and s2 == s and np.array_equal(b2, b)
    assert CC.position_key(ob[0], int(os_[0])) == ((O.zhash(ob[0], int(os_[0])) & ~CC.BUSY) or 1)
    assert all(CC.position_key(b, int(s)) < CC.BUSY for b, s in zip(ob, os_))
    assert CC.position_key(ob[0], int(os_[0]), CC.key_mask(11)) < (1 << 24)


def test_verifier_accepts_a_correct_table(table):
    d, ref = table
    st = CC.check_xcache(d, ref)
    assert st["entries"] == len(_entries(d)) >= 60 and st["duplicates"] == 0
    assert len(_entries(d, lambda c: c > 64)) >= 4
    assert (d["board"][_entries(d), 11] >> 28).tolist().count(1) >= 40     # black to move


def _mutants(d):
    """(name, mutated copy) for every tear a racing filing can produce."""
    ents = _entries(d)
    long_ = _entries(d, lambda c: c > 64)
    a = ents[1]
    b = next(e for e in ents if not np.array_equal(d["label"][e], d["label"][a]))     # other labels, priors and value
    la, lb = long_[0], long_[1]
    assert not np.array_equal(d["label"][la, 64:], d["label"][lb, 64:])
    out = []

    def mut(name, f):
        m = {k: v.copy() for k, v in d.items()}
        f(m)
        out.append((name, m))
    mut("labels of another entry", lambda m: m["label"].__setitem__(a, d["label"][b]))
    mut("labels 64..127 of another entry", lambda m: m["label"][la].__setitem__(slice(64, 128), d["label"][lb, 64:]))
    mut("priors of another entry", lambda m: m["P"].__setitem__(a, d["P"][b]))
    c = next(e for e in ents if d["count"][e] != d["count"][a])
    mut("count of another entry", lambda m: m["count"].__setitem__(a, d["count"][c]))
    v = next(e for e in ents if d["value"][e] != d["value"][a])
    mut("value of another entry", lambda m: m["value"].__setitem__(a, d["value"][v]))
    mut("wrong key", lambda m: m["key"].__setitem__(a, np.uint64(int(d["key"][a]) ^ 2)))

    def move_bucket(m):
        src = a
        dst = next(e for e in range(len(d["key"])) if d["key"][e] == 0 and e // 64 != src // 64)
        for k in m:
            m[k][dst] = d[k][src]
        m["key"][src] = 0
    mut("wrong bucket", move_bucket)
    mut("flipped side bit", lambda m: m["board"][a].__setitem__(11, d["board"][a, 11] ^ np.uint32(1 << 28)))
    empty = next(e for e in range(len(d["key"])) if d["key"][e] == 0)
    mut("leftover claim (empty slot)", lambda m: m["key"].__setitem__(empty, np.uint64(CC.BUSY | int(d["key"][a]))))
    mut("leftover claim (live entry)", lambda m: m["key"].__setitem__(b, np.uint64(CC.BUSY | int(d["key"][b]))))
    return out


def test_verifier_rejects_every_torn_entry(table):
    d, ref = table
    muts = _mutants(d)
    assert len(muts) == 10
    for name, m in muts:
        with pytest.raises(AssertionError):
            CC.check_xcache(m, ref)
            pytest.fail("the verifier accepted: %s" % name)


def test_verifier_reports_duplicates(table):
    d, ref = table
    m = {k: v.copy() for k, v in d.items()}
    a = _entries(d)[0]
    dst = next(e for e in range(len(d["key"])) if d["key"][e] == 0 and e // 64 == a // 64)
    for k in m:
        m[k][dst] = d[k][a]
    assert CC.check_xcache(m, ref)["duplicates"] == 1


def test_per_tree_verifier_on_an_oracle_tree():
    """check_eval_cache against a per-tree table built from an oracle tree: correct entries pass; an entry whose node, value,
    board or key belongs to another node is rejected."""
    fwd = fakenet.make_forward("signed", 5)
    b0 = O.fen_to_board(O.START_FEN)
    S = O.Search(1, 20000)
    S.reset(b0[None], np.array([1], np.uint8), None)     # black to move at the root: the side alternates from 1
    for step in range(41):
        p, _ = S.select(0 if step == 0 else 1)
        S.expand_backup(*fwd(p))
    tree = S.tree_dump(0)
    ref = CC.Reference(CC.oracle_expander(fwd))
    par = CC._record_parents(tree)
    recs = [-1] + [r for r in range(len(tree)) if tree[r, 6] >= 0]
    ec = dict(key=np.zeros(8192, np.uint64), node=np.zeros(8192, np.int32), value=np.zeros(8192, np.float32),
              board=np.zeros((8192, 12), np.uint32), record=np.full(8192, -2, np.int32))
    fill = np.zeros(128, np.int64)
    for r in recs:
        path, q = [], r
        while q >= 0:
            path.append(int(tree[q, 1]))
            q = int(par[q])
        b = b0.copy()
        for lab in reversed(path):
            b = O.apply_move(b, lab)[0]
        s = 1 ^ (len(path) & 1)
        k = CC.position_key(b, s)
        bk = (k >> 17) & 127
        i = bk * 64 + fill[bk]
        fill[bk] += 1
        ec["key"][i], ec["node"][i], ec["record"][i] = k, 1000 + r, r
        ec["board"][i] = CC.pack_board(b, s)
        ec["value"][i] = ref.get([(b, s)])[0][3]
    assert len(recs) >= 30
    assert CC.check_eval_cache(ec, tree, b0, 1, ref) == len(recs)
    live = np.nonzero(ec["key"])[0]
    i, j = int(live[3]), int(live[-1])
    for name, f in [("record of another node", lambda m: m["record"].__setitem__(i, ec["record"][j])),
                    ("value of another node", lambda m: m["value"].__setitem__(i, ec["value"][j])),
                    ("board of another node", lambda m: m["board"].__setitem__(i, ec["board"][j])),
                    ("node not in the tree", lambda m: m["record"].__setitem__(i, -2))]:
        m = {k: v.copy() for k, v in ec.items()}
        f(m)
        with pytest.raises(AssertionError):
            CC.check_eval_cache(m, tree, b0, 1, ref)
            pytest.fail("the per-tree verifier accepted: %s" % name)
