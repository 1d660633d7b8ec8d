"""The UCCI protocol loop (cchess_zero_amd.ucci.UcciEngine) against a searcher built here from the C oracle's search, fakenet,
the lines model and the king-safe model: no GPU.  (The host tables come from libcchess_hip.so, which the build leaves in the
tree.)"""
import io

import numpy as np
import pytest

import fakenet
import kingsafe_model as KM
import lines_model as LM
from cchess_zero_amd import notation
from oracle import oracle as O

MATED = "R3k4/1R7/9/9/9/9/9/9/9/3K5 b"   # black: the rook on a9 checks along the back rank, b8 holds rank 8, the kings face on d


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__
    __graft_entry__.build_hip_only()


class OracleSearcher:
    """The searcher interface of UcciEngine on one oracle tree."""
    width = 1

    def __init__(self, salt=5):
        self.s, self.fwd = O.Search(1, 20000), fakenet.make_forward("pos", salt)
        self.pos, self.rooted, self.resets = None, False, 0

    def set_position(self, board, side, rr):
        self.pos, self.rooted = (np.array(board, np.uint8), int(side), int(rr)), False

    def kingsafe_mask(self):
        safe, flags = KM.kingsafe(self.pos[0], self.pos[1])
        return KM.mask_of(safe), int(flags)

    def _step(self, mode):
        planes, _ = self.s.select(mode)
        self.s.expand_backup(*self.fwd(planes))

    def _root(self):
        if not self.rooted:
            b, s, rr = self.pos
            self.s.reset(b[None], np.array([s], np.uint8), np.array([rr], np.int32))
            self._step(0)
            self.rooted, self.resets = True, self.resets + 1

    def search(self, playouts):
        self._root()
        for _ in range(playouts):
            self._step(1)
        return playouts

    def lines(self, allowed, n_lines, max_len):
        self._root()
        m, v, q, l = LM.lines_from_dump(self.s.tree_dump(0), LM.mask_labels(allowed), n_lines, max_len)
        return [dict(pv=[int(x) for x in m[j, :l[j]]], visits=[int(x) for x in v[j, :l[j]]], q=[float(x) for x in q[j, :l[j]]])
                for j in range(n_lines) if l[j]]


def _session(script, searcher=None, **kw):
    from cchess_zero_amd.ucci import UcciEngine
    out = io.StringIO()
    eng = UcciEngine(searcher or OracleSearcher(), io.StringIO(script), out, **kw)
    eng.run()
    return out.getvalue().splitlines(), eng


def _after(*moves):
    """The position after `moves` from the start, by the oracle."""
    b, s, rr = O.fen_to_board(O.START_FEN), 0, 0
    for m in moves:
        b, cap, _ = O.apply_move(b, O.labels().index(m))
        s, rr = s ^ 1, 0 if cap else rr + 1
    return b, s, rr


def _model_lines(pos, playouts, n_lines, ban=(), max_len=16):
    """The model's lines of a fresh oracle search of pos: [(move texts, visits of the first move, q of the first move)]."""
    ref = OracleSearcher()
    ref.set_position(*pos)
    ref.search(playouts)
    safe = [int(l) for l in KM.kingsafe(pos[0], pos[1])[0] if O.labels()[int(l)] not in ban]
    L = O.labels()
    return [([L[m] for m in ln["pv"]], ln["visits"][0], ln["q"][0]) for ln in ref.lines(KM.mask_of(safe), n_lines, max_len)], [L[l] for l in safe]


def test_scripted_session():
    lines, eng = _session("ucci\nisready\nposition startpos moves h2e2\ngo nodes 48\nquit\n")
    assert lines[0].startswith("id name ") and lines[1].startswith("id author ")
    assert lines[2].startswith("option Playouts type spin ") and lines[3] == "option MultiPV type spin min 1 max 8 default 1"
    assert lines[4:6] == ["ucciok", "readyok"] and lines[-1] == "bye"
    pos = _after("h2e2")
    assert np.array_equal(eng.pos[0], pos[0]) and eng.pos[1:] == (1, 1)
    want, safe = _model_lines(pos, 48, 1)
    info = [l for l in lines if l.startswith("info depth")]
    best = [l for l in lines if l.startswith("bestmove")]
    assert len(info) == 1 and len(best) == 1 and lines.index(info[0]) < lines.index(best[0])
    tok = info[0].split()
    pv = tok[tok.index("pv") + 1:]
    assert pv == want[0][0] and int(tok[tok.index("depth") + 1]) == len(pv) and "multipv" not in tok
    assert int(tok[tok.index("score") + 1]) == int(round(1000.0 * want[0][2])) and int(tok[tok.index("nodes") + 1]) == 48
    b = best[0].split()
    assert b[1] == pv[0] and b[1] in safe
    assert b[2:] == (["ponder", pv[1]] if len(pv) > 1 else [])


def test_multipv_gives_the_lines_in_rank_order():
    lines, _ = _session("setoption MultiPV 3\nposition startpos moves h2e2\ngo nodes 48\nquit\n")
    want, _ = _model_lines(_after("h2e2"), 48, 3)
    info = [l.split() for l in lines if l.startswith("info depth")]
    assert len(info) == 3 and [int(t[t.index("multipv") + 1]) for t in info] == [1, 2, 3]
    assert [t[t.index("pv") + 1:] for t in info] == [w[0] for w in want]
    assert want[0][1] >= want[1][1] >= want[2][1]
    assert [l for l in lines if l.startswith("bestmove")][0].split()[1] == want[0][0][0]
    # the option's range, and a bare go
    lines, eng = _session("setoption MultiPV 99\nsetoption Playouts 24\ngo\nquit\n")
    assert eng.options == dict(playouts=24, multipv=8) and len([l for l in lines if l.startswith("info depth")]) == 8
    assert all(int(l.split()[l.split().index("nodes") + 1]) == 24 for l in lines if l.startswith("info depth"))


def test_banmoves_plays_another_move_until_the_next_position():
    first, _ = _model_lines(_after("h2e2"), 48, 1)
    best = first[0][0][0]
    lines, eng = _session("position startpos moves h2e2\nbanmoves %s\ngo nodes 48\nposition startpos moves h2e2\ngo nodes 48\nquit\n" % best)
    played = [l.split()[1] for l in lines if l.startswith("bestmove")]
    want, _ = _model_lines(_after("h2e2"), 48, 1, ban=(best,))
    assert played == [want[0][0][0], best] and played[0] != best and eng.ban == []


def test_illegal_move_and_bad_fen_keep_the_position():
    from cchess_zero_amd.ucci import UcciEngine
    out = io.StringIO()
    eng = UcciEngine(OracleSearcher(), io.StringIO(""), out)
    eng.handle("position startpos moves h2e2")
    eng.handle("banmoves h7e7")
    kept = (eng.pos[0].copy(), eng.pos[1], eng.pos[2], list(eng.ban))
    for bad in ("position startpos moves a0a9",            # the rook's own pawn is in the way
                "position startpos moves h2e2 h2e2",         # the cannon is gone from h2
                "position startpos moves z9z9",              # no move of the board
                "position fen rnbakabnr/9/1c5c1 w",          # three ranks
                "position fen 4k4/4R4/9/9/9/9/9/9/9/3K5 b moves e9d9",   # out of the rook's check onto the file of the red king: not king-safe
                "position elsewhere"):
        n = len(out.getvalue().splitlines())
        eng.handle(bad)
        said = out.getvalue().splitlines()[n:]
        assert len(said) == 1 and said[0].startswith("info string "), (bad, said)
        assert np.array_equal(eng.pos[0], kept[0]) and (eng.pos[1], eng.pos[2], eng.ban) == kept[1:], bad
        assert np.array_equal(eng.searcher.pos[0], kept[0]) and eng.searcher.pos[1] == kept[1]
    # the restrict round follows captures: the cannon takes the knight on h9
    eng.handle("position startpos moves h2h9")
    assert eng.pos[2] == 0 and eng.pos[1] == 1 and eng.ban == []
    eng.handle("position fen %s - - 7 20 moves h2e2" % notation.START_FEN)
    assert eng.pos[2] == 8
    eng.handle("frobnicate 1 2 3")    # unknown commands are ignored
    eng.handle("stop")
    assert len(out.getvalue().splitlines()) == n + 1


def test_mated_position_answers_nobestmove():
    board, side, _ = notation.fen_to_position(MATED)
    assert KM.kingsafe(board, side)[1] & KM.NO_SAFE_MOVE and KM.kingsafe(board, side)[1] & KM.IN_CHECK
    s = OracleSearcher()
    lines, _ = _session("position fen %s\ngo nodes 16\nquit\n" % MATED, searcher=s)
    assert lines == ["nobestmove", "bye"] and s.resets == 0    # not searched
    # every king-safe move banned: the same answer
    pos = notation.fen_to_position("4k4/9/9/9/9/9/9/9/4R4/3K5 b")
    safe = [O.labels()[int(l)] for l in KM.kingsafe(pos[0], pos[1])[0]]
    assert safe
    lines, _ = _session("position fen 4k4/9/9/9/9/9/9/9/4R4/3K5 b\nbanmoves %s\ngo nodes 8\nquit\n" % " ".join(safe))
    assert lines == ["nobestmove", "bye"]


def test_go_time_depth_and_stop():
    from cchess_zero_amd.ucci import CHUNK_STEPS
    ticks = iter(range(10 ** 6))
    clock = lambda: next(ticks) * 0.040    # every look at the clock is 40 ms later
    # go time 100: start at 0; after chunk 1 the clock reads 40 ms (< 90), after chunk 2 80 ms, after chunk 3 120 ms -> three chunks
    lines, _ = _session("go time 100\nquit\n", clock=clock)
    tok = [l for l in lines if l.startswith("info depth")][0].split()
    assert int(tok[tok.index("nodes") + 1]) == 3 * CHUNK_STEPS
    # go time 1 still runs one chunk
    lines, _ = _session("go time 1\nquit\n", clock=clock)
    tok = [l for l in lines if l.startswith("info depth")][0].split()
    assert int(tok[tok.index("nodes") + 1]) == CHUNK_STEPS
    # go depth D: chunks until line 0 is D long or Playouts is reached
    lines, _ = _session("setoption Playouts 200\ngo depth 2\nquit\n")
    tok = [l for l in lines if l.startswith("info depth")][0].split()
    nodes, depth = int(tok[tok.index("nodes") + 1]), int(tok[tok.index("depth") + 1])
    assert (depth >= 2 and nodes % CHUNK_STEPS == 0 and nodes < 200) or nodes == 200
    lines, _ = _session("setoption Playouts 40\ngo depth 60\nquit\n")
    tok = [l for l in lines if l.startswith("info depth")][0].split()
    assert int(tok[tok.index("nodes") + 1]) == 40
    # stop, already waiting when the first chunk ends, ends a long search; isready is answered meanwhile, quit waits its turn
    from cchess_zero_amd.ucci import UcciEngine
    out = io.StringIO()
    eng = UcciEngine(OracleSearcher(), io.StringIO(""), out)
    for l in ("isready\n", "stop\n", "quit\n"):
        eng._lines.put(l)
    eng.go(["nodes", "100000"])
    said = out.getvalue().splitlines()
    assert said[0] == "readyok" and said[-1].startswith("bestmove ")
    tok = said[1].split()
    assert int(tok[tok.index("nodes") + 1]) == CHUNK_STEPS and eng._lines.get_nowait() == "quit\n"
