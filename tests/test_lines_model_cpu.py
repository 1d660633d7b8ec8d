"""The model of cz_search_lines (tests/lines_model.py) on hand-written dumps — one per rule —, on the reference's golden
searches and on the C oracle's trees; standard FEN in cchess_zero_amd.notation.  CPU only."""
import numpy as np
import pytest

import fakenet
import lines_cases
import lines_model as LM
import searchdrive
from cchess_zero_amd import notation
from oracle import oracle as O


def _dump(*records):
    """records (depth, label, N, q, child_count) -> a dump array; W and P are not read by the model."""
    out = np.zeros((len(records), 7), np.int32)
    for k, (d, label, n, q, cc) in enumerate(records):
        out[k] = (d, label, n, 0, np.float32(q).view(np.int32), 0, cc)
    return out


def _lines(rec, allowed=None, n_lines=3, max_len=4):
    m, v, q, l = LM.lines_from_dump(rec, allowed, n_lines, max_len)
    return [([int(x) for x in m[j, :l[j]]], [int(x) for x in v[j, :l[j]]]) for j in range(n_lines)], (m, v, q, l)


def test_root_tie_goes_to_the_earlier_child():
    rec = _dump((0, 10, 5, 0.1, -1), (0, 11, 5, 0.9, -1), (0, 12, 7, 0.2, -1), (0, 13, 5, 0.3, -1))
    got, _ = _lines(rec, n_lines=4)
    assert [g[0] for g in got] == [[12], [10], [11], [13]]


def test_tie_below_the_root_goes_to_the_earlier_child():
    rec = _dump((0, 10, 9, 0.5, 3), (1, 20, 2, 0.1, -1), (1, 21, 4, 0.2, -1), (1, 22, 4, 0.3, 1), (2, 30, 3, 0.0, -1), (0, 11, 1, 0.0, -1))
    got, (m, v, q, l) = _lines(rec)
    assert got[0] == ([10, 21], [9, 4]) and got[1] == ([11], [1]) and got[2] == ([], [])
    assert q[0, 0].view(np.int32) == np.float32(0.5).view(np.int32) and q[0, 1] == np.float32(0.2)
    assert m[0, 2] == 0xFFFF and v[0, 2] == 0 and q[0, 2].view(np.int32) == 0


def test_best_child_without_a_visit_ends_the_line():
    rec = _dump((0, 10, 3, 0.5, 2), (1, 20, 0, 0.0, -1), (1, 21, 0, 0.0, -1), (0, 11, 0, 0.0, -1))
    got, _ = _lines(rec)
    assert got[0] == ([10], [3])
    assert got[1] == ([11], [0])     # a candidate without a visit still gives a line of length 1
    # a negative count (a pending descent's virtual loss is never in N, but N <= 0 is the rule) stops too
    rec[1, LM.N] = -1
    assert _lines(rec)[0][0] == ([10], [3])


def test_unexpanded_root_has_no_lines():
    """An unexpanded root (and a root without children) dumps no record: every line is empty, every element is written."""
    m, v, q, l = LM.lines_from_dump(np.zeros((0, 7), np.int32), None, 2, 3)
    assert not l.any() and (m == 0xFFFF).all() and not v.any() and not q.view(np.int32).any()
    assert m.shape == v.shape == q.shape == (2, 3) and l.shape == (2,)
    assert m.dtype == np.uint16 and v.dtype == np.int32 and q.dtype == np.float32 and l.dtype == np.uint16


def test_mask_removes_the_most_visited_child():
    rec = _dump((0, 10, 9, 0.5, 1), (1, 20, 8, 0.1, -1), (0, 11, 2, 0.0, -1), (0, 12, 2, 0.0, -1))
    assert _lines(rec)[0][0] == ([10, 20], [9, 8])
    got, _ = _lines(rec, allowed=[11, 12, 99])
    assert [g[0] for g in got] == [[11], [12], []]
    assert [g[0] for g in _lines(rec, allowed=[])[0]] == [[], [], []]


def test_more_lines_than_candidates():
    rec = _dump((0, 10, 1, 0.0, -1), (0, 11, 2, 0.0, -1))
    m, v, q, l = LM.lines_from_dump(rec, None, 128, 2)
    assert list(l[:3]) == [1, 1, 0] and not l[2:].any() and (m[2:] == 0xFFFF).all() and list(m[:2, 0]) == [11, 10]


def test_truncation_at_max_len():
    chain = [(d, 100 + d, 10 - d, 0.0, 1) for d in range(6)]
    chain[-1] = (5, 105, 5, 0.0, -1)
    rec = _dump(*chain)
    assert _lines(rec, n_lines=1, max_len=8)[0][0][0] == [100, 101, 102, 103, 104, 105]
    assert _lines(rec, n_lines=1, max_len=4)[0][0][0] == [100, 101, 102, 103]
    assert _lines(rec, n_lines=1, max_len=1)[0][0][0] == [100]


def test_mask_labels_round_trip():
    import kingsafe_model
    labels = [0, 31, 32, 2085]
    assert LM.mask_labels(kingsafe_model.mask_of(labels)) == labels
    assert LM.mask_labels(kingsafe_model.mask_of(labels).view(np.int32)) == labels


class _PerTreeOracle:
    """One oracle search per tree (the cases have different playout counts); keeps every dump searchdrive asks for."""

    def __init__(self, G):
        self.G, self.e, self.dumps = G, [O.Search(1, 200000) for _ in range(G)], [[] for _ in range(G)]

    def reset(self, boards, side, rr):
        for g in range(self.G):
            self.e[g].reset(boards[g:g + 1], side[g:g + 1], rr[g:g + 1])

    def select(self, mode, mask=None):
        planes, need = np.zeros((self.G, 9, 10, 14), np.float32), np.zeros(self.G, np.uint8)
        self._ran = [mask is None or bool(mask[g]) for g in range(self.G)]
        for g in range(self.G):
            if self._ran[g]:
                p, n = self.e[g].select(mode)
                planes[g], need[g] = p[0], n[0]
        return planes, need

    def expand_backup(self, logits, value):
        for g in range(self.G):
            if self._ran[g]:
                self.e[g].expand_backup(logits[g:g + 1], value[g:g + 1])

    def root_stats(self):
        st = [e.root_stats() for e in self.e]
        return {k: np.concatenate([s[k] for s in st]) for k in st[0]}

    def advance(self, played):
        for g in range(self.G):
            self.e[g].advance(played[g:g + 1])

    def tree_dump(self, g):
        self.dumps[g].append(self.e[g].tree_dump(0))
        return self.dumps[g][-1]


def test_line_zero_starts_at_the_golden_first_maximum(mcts_golden):
    """On every ply of the reference's golden searches, line 0 of the model (over the oracle's tree, whose digest the golden
    pins) starts with the first maximum of N of the reference's own root list, with that child's N and Q bits."""
    cases = mcts_golden["cases"]
    eng = _PerTreeOracle(len(cases))
    results, logs = searchdrive.run_cases(eng, cases)
    searchdrive.check_against_golden(results, logs, cases)
    plies = 0
    for g, c in enumerate(cases):
        for ply, gp in enumerate(c["plies"]):
            root = gp["root"]
            best = LM.first_max([r[1] for r in root])
            m, v, q, l = LM.lines_from_dump(eng.dumps[g][ply], None, 2, 8)
            assert l[0] >= 1 and (int(m[0, 0]), int(v[0, 0]), int(q[0, 0].view(np.uint32))) == (root[best][0], root[best][1], root[best][3])
            assert len(root) < 2 or v[1, 0] <= v[0, 0]
            plies += 1
    assert plies >= 24


@pytest.fixture(scope="module")
def oracle_trees(rules_golden):
    """64 corpus trees after 1 + 48 lock-steps (fakenet pos, salt 99) on the C oracle: (boards, side, dumps)."""
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    orc = O.Search(64, 20000)
    orc.reset(boards, side, rr)
    lines_cases.run_ply(orc, fakenet.make_forward("pos", 99), 48)
    return boards, side, [orc.tree_dump(g) for g in range(64)]


def test_model_lines_replay_legally_on_oracle_trees(oracle_trees):
    boards, side, dumps = oracle_trees
    assert int(side.sum()) == 32    # half the roots are black to move
    longest = ties = 0
    for g in range(64):
        m, v, q, l = LM.lines_from_dump(dumps[g], None, 5, 8)
        ties += int(l[1] > 0 and v[0, 0] == v[1, 0])
        assert l[0] >= 1 and all(v[j, 0] >= v[j + 1, 0] for j in range(4))
        for j in range(5):
            b, s = boards[g], int(side[g])
            for i in range(int(l[j])):
                assert int(m[j, i]) in O.legal_moves(b, s), (g, j, i)
                b, s = O.apply_move(b, int(m[j, i]))[0], s ^ 1
            longest = max(longest, int(l[j]))
            assert (m[j, l[j]:] == 0xFFFF).all() and not v[j, l[j]:].any()
    assert longest == 4 and ties == 2


def test_long_lines_on_oracle_trees(rules_golden):
    """fakenet mode deep digs one line: principal lines of 10-28 moves, which max_len = 16 truncates for six of the eight."""
    boards, side, rr = lines_cases.corpus(rules_golden, 64)
    orc = O.Search(8, 20000)
    orc.reset(boards[:8], side[:8], rr[:8])
    lines_cases.run_ply(orc, fakenet.make_forward("deep", 913), 96)
    full = [LM.lines_from_dump(orc.tree_dump(g), None, 3, 64) for g in range(8)]
    cut = [LM.lines_from_dump(orc.tree_dump(g), None, 3, 16) for g in range(8)]
    assert [int(x[3][0]) for x in full] == [20, 24, 28, 10, 23, 23, 14, 23]
    assert [int(x[3][0]) for x in cut] == [16, 16, 16, 10, 16, 16, 14, 16]
    for a, b in zip(full, cut):
        assert np.array_equal(a[0][:, :16], b[0]) and np.array_equal(a[1][:, :16], b[1])


# ---- standard FEN -----------------------------------------------------------------------------------------------------
START = "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR w"
AFTER_H2E2 = "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C2C4/9/RNBAKABNR b"


def test_fen_fixed_vectors():
    board, side, rr = notation.fen_to_position(START)
    assert np.array_equal(board, notation.state_to_board(notation.START_STATE)) and (side, rr) == (0, 0)
    assert np.array_equal(board, O.fen_to_board(O.START_FEN))
    label = O.labels().index("h2e2")
    after = O.apply_move(board, label)[0]
    assert " ".join(notation.position_to_fen(after, 1).split()[:2]) == AFTER_H2E2   # rank order and file direction, not a mirror
    b2, s2, _ = notation.fen_to_position(AFTER_H2E2)
    assert np.array_equal(b2, after) and s2 == 1


def test_fen_round_trips(rules_golden):
    g = rules_golden
    n = 0
    for i in range(0, len(g["boards"]), 7):
        b, s = g["boards"][i], int(g["side"][i])
        if not ((b == 1).any() and (b == 8).any()):
            continue
        fen = notation.position_to_fen(b, s, rr=i % 60, fullmove=1 + i // 2)
        b2, s2, rr2 = notation.fen_to_position(fen)
        assert np.array_equal(b, b2) and s2 == s and rr2 == i % 60 and fen.split()[5] == str(1 + i // 2)
        assert notation.position_to_fen(b2, s2, rr2, 1 + i // 2) == fen
        n += 1
    assert n > 50
    # side letters, optional fields, E / H for B / N
    assert notation.fen_to_position(START[:-2] + " r")[1] == 0 and notation.fen_to_position(START[:-2] + " b - - 12 30")[1:] == (1, 12)
    assert notation.fen_to_position(START[:-2])[1] == 0
    eh = START.replace("b", "e").replace("n", "h").replace("B", "E").replace("N", "H")
    assert np.array_equal(notation.fen_to_position(eh)[0], notation.fen_to_position(START)[0])


@pytest.mark.parametrize("fen", [
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9 w",                    # nine ranks
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/9/RNBAKABNR w",        # eleven
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C2/9/RNBAKABNR w",          # a rank of ten files
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/8/P1P1P1P1P/1C5C1/9/RNBAKABNR w",          # a rank of eight
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBQKABNR w",          # an unknown letter
    "rnba1abnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR w",          # no black king
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBA1ABNR w",          # no red king
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR x",          # no such side
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/9/RNBAKABNR w - - x 1",  # a clock that is no number
    "rnbakabnr/9/1c5c1/p1p1p1p1p/9/9/P1P1P1P1P/1C5C1/0RNBAKABNR/9 w",         # a zero run
    "", 7])
def test_malformed_fen_raises(fen):
    with pytest.raises(ValueError):
        notation.fen_to_position(fen)
