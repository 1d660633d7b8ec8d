"""The host side of the opening book without a GPU: Book's reduce / merge / save / load / stats fed with tests/book_model.py's
tuples, the command lines' argument errors, the UCCI engine's Book options on a fake searcher (tests/test_ucci_cpu.py's, extended),
and the book kernels' code-object metadata (no scratch)."""
import io
import json
import os
import re
import subprocess

import numpy as np
import pytest

import book_model as BM
from oracle import oracle as O
from cchess_zero_amd.notation import START_FEN
from test_ucci_cpu import OracleSearcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = [(["h2e2", "h9g7", "h0g2", "i9h9", "i0h0", "b9c7"], 1), (["b2e2", "b9c7", "b0c2", "a9b9"], 0), (["h2e2", "b9c7", "h0g2"], -1),
         (["c3c4", "h9g7"], 1), (["h2e2", "h9g7", "b0c2"], 0)]


@pytest.fixture(scope="module", autouse=True)
def _library():
    import __graft_entry__
    __graft_entry__.build_hip_only()


def _records(games):
    return np.concatenate([BM.records_of_game(m, r) for m, r in games])


def _book(games, max_ply=40):
    from cchess_zero_amd.book import Book
    rec = _records(games)
    return Book().set_entries(*BM.entries(rec, max_ply), rules="capture", max_ply=max_ply, source_games=len(games), source_plies=len(rec))


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_reduce_and_merge_equal_the_model():
    whole = _book(GAMES)
    assert _same(whole.arrays(), BM.book_of(_records(GAMES), 40)) and len(whole) > 8
    a, b = _book(GAMES[:2]), _book(GAMES[2:])
    m = a.merge(b)
    assert _same(m.arrays(), BM.merge(a.arrays(), b.arrays())) and _same(m.arrays(), whole.arrays())
    assert (m.source_games, m.source_plies, m.rules, m.max_ply) == (5, len(_records(GAMES)), "capture", 40)
    assert _same(b.merge(a).arrays(), m.arrays())
    from cchess_zero_amd.book import Book
    assert _same(Book().merge(whole).arrays(), whole.arrays())
    with pytest.raises(ValueError):
        whole.merge(Book().set_entries(*BM.entries(_records(GAMES[:1]), 40), rules="xiangqi"))
    # max_ply: the records at or beyond it are no entries
    assert _same(_book(GAMES, 2).arrays(), BM.book_of(_records(GAMES), 2)) and len(_book(GAMES, 2)) < len(whole)


def test_save_and_load_round_trip_byte_for_byte(tmp_path):
    from cchess_zero_amd.book import Book
    bk = _book(GAMES)
    p, q = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    bk.save(p)
    back = Book().load(p)
    assert _same(back.arrays(), bk.arrays()) and (back.rules, back.max_ply, back.source_games, back.source_plies) == ("capture", 40, 5, bk.source_plies)
    back.save(q)
    assert open(p, "rb").read() == open(q, "rb").read()
    # a game and its mirrored twin: the same file
    twin = [(BM.mirror_moves(m), r) for m, r in GAMES]
    _book(twin).save(q)
    assert open(p, "rb").read() == open(q, "rb").read()
    z = np.load(p)
    assert sorted(z.files) == ["draws", "games", "key", "label", "meta", "wins"] and z["key"].dtype == np.uint64 and z["label"].dtype == np.uint16
    assert z["games"].dtype == z["wins"].dtype == z["draws"].dtype == np.uint32


def _write(path, bk, **change):
    d = dict(zip(("key", "label", "games", "wins", "draws"), bk.arrays()), meta=np.array([1, 0, 40, 5, 16], np.int64))
    d.update(change)
    np.savez(path, **d)


def test_load_refuses_what_is_no_book(tmp_path):
    from cchess_zero_amd.book import Book
    bk = _book(GAMES)
    p = str(tmp_path / "x.npz")
    _write(p, bk)
    assert _same(Book().load(p).arrays(), bk.arrays())
    n = len(bk)
    swap = np.arange(n)
    swap[[0, n - 1]] = swap[[n - 1, 0]]
    twice = np.concatenate([np.arange(n), [n - 1]])
    for change in (dict(zip(("key", "label", "games", "wins", "draws"), (a[swap] for a in bk.arrays()))),          # unsorted
                   dict(zip(("key", "label", "games", "wins", "draws"), (a[twice] for a in bk.arrays()))),         # a pair twice
                   dict(key=bk.key.astype(np.int64)), dict(games=bk.games[:-1]), dict(label=np.full(n, 2086, np.uint16)),
                   dict(wins=bk.games + 1), dict(games=np.zeros(n, np.uint32)), dict(meta=np.array([9, 0, 40, 5, 16], np.int64))):
        _write(p, bk, **change)
        with pytest.raises(ValueError):
            Book().load(p)
    # label order inside one key
    lo, hi = bk.entries_of(BM.canonical(O.fen_to_board(O.START_FEN), 0)[0])
    assert hi - lo == 2
    lab = bk.label.copy()
    lab[[lo, lo + 1]] = lab[[lo + 1, lo]]
    _write(p, bk, label=lab)
    with pytest.raises(ValueError):
        Book().load(p)


def test_the_games_of_one_position_stay_below_2_to_the_32(tmp_path):
    from cchess_zero_amd.book import Book, check_table
    key, label = np.array([5, 5, 9], np.uint64), np.array([1, 2, 0], np.uint16)
    zero = np.zeros(3, np.uint32)
    ok = np.array([2 ** 31, 2 ** 31 - 1, 2 ** 32 - 1], np.uint32)
    check_table(key, label, ok, zero, zero)
    bad = np.array([2 ** 31, 2 ** 31, 1], np.uint32)
    with pytest.raises(ValueError):
        check_table(key, label, bad, zero, zero)
    p = str(tmp_path / "big.npz")
    np.savez(p, key=key, label=label, games=bad, wins=zero, draws=zero, meta=np.array([1, 1, 40, 0, 0], np.int64))
    with pytest.raises(ValueError):
        Book().load(p)
    half = Book()._set(key[:1], label[:1], ok[:1], zero[:1], zero[:1])
    with pytest.raises(ValueError):
        half.merge(half)                                                     # one entry of 2^32 games
    other = Book()._set(key[:1], label[1:2], ok[:1], zero[:1], zero[:1])
    with pytest.raises(ValueError):
        half.merge(other)                                                    # two entries of one position


def test_stats():
    s = _book(GAMES).stats()
    assert s["entries"] == len(_book(GAMES)) and s["positions"] == len(set(BM.book_of(_records(GAMES), 40)[0].tolist()))
    assert s["games_at_ply0"] == 5 and len(s["deepest_line"]) == 6
    assert s["deepest_line"] in (GAMES[0][0], BM.mirror_moves(GAMES[0][0]))
    # game 1 is the mirror image of the first four plies of game 0: those four moves have two games or more, the fifth has one
    two = _book(GAMES).stats(min_games=2)["deepest_line"]
    assert two in (GAMES[0][0][:4], GAMES[1][0])
    assert _book(GAMES).stats(min_games=6)["deepest_line"] == []


def test_command_line_argument_errors(tmp_path, capsys):
    from cchess_zero_amd import arena, book
    missing = str(tmp_path / "none.npz")
    for argv in ([], ["--build", "--probe"], ["--build", "--in", "x.pgn"], ["--build", "--out", "b.npz"], ["--probe", "--fen", START_FEN],
                 ["--stats"], ["--probe", "--book", missing, "--fen", START_FEN], ["--stats", "--book", missing],
                 ["--build", "--in", "x.pgn", "--out", "b.npz", "--notation", "wxf"], ["--build", "--in", "x.pgn", "--out", "b.npz", "--max_ply", "-1"],
                 ["--build", "--in", "x.pgn", "--out", "b.npz", "--merge", missing], ["--build", "--in", "x.pgn", "--out", "b.npz", "--rules", "chess"]):
        with pytest.raises(SystemExit) as e:
            book.main(argv)
        assert e.value.code == 2, argv
    p = str(tmp_path / "b.npz")
    _book(GAMES).save(p)
    for argv in (["--probe", "--book", p], ["--probe", "--book", p, "--fen", "9/9 w"], ["--probe", "--book", p, "--fen", START_FEN, "--notation", "any"],
                 ["--build", "--in", "x.pgn", "--out", "b.npz", "--merge", p]):      # the last: a capture book into a xiangqi build
        with pytest.raises(SystemExit) as e:
            book.main(argv)
        assert e.value.code == 2, argv
    with pytest.raises(SystemExit) as e:
        arena.main(["--all_openings", "--book", p])
    assert e.value.code == 2 and "--all_openings and --book" in capsys.readouterr().err
    assert book.main(["--stats", "--book", p]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["games_at_ply0"] == 5


# ---- UCCI ---------------------------------------------------------------------------------------------------------------------
class BookSearcher(OracleSearcher):
    """OracleSearcher with the optional book / tablebase / mate calls, the book answered by the model from the host table."""

    def __init__(self, tb=None, mate_line=None):
        super().__init__()
        self.calls, self.tb, self.mate_line = [], tb, mate_line

    def book(self, file, allowed, min_games, sample):
        from cchess_zero_amd.book import Book
        self.calls.append(("book", file, int(min_games), bool(sample)))
        bk = Book().load(file)
        played, index = BM.choose(bk.arrays(), self.pos[0][None], [self.pos[1]], np.asarray(allowed, np.uint32)[None], int(min_games), 1 if sample else 0,
                                  [0x80000000])
        if int(index[0]) < 0:
            return None
        i = int(index[0])
        n, w, d = int(bk.games[i]), int(bk.wins[i]), int(bk.draws[i])
        return int(played[0]), dict(games=n, wins=w, draws=d, losses=n - w - d, score=(w + d / 2.0) / n)

    def tablebase(self, directory):
        self.calls.append(("tablebase", directory))
        return self.tb

    def mate(self, plies):
        self.calls.append(("mate", plies))
        return self.mate_line


def _session(script, searcher):
    from cchess_zero_amd.ucci import UcciEngine
    out = io.StringIO()
    UcciEngine(searcher, io.StringIO(script), out, clock=lambda: 0.0).run()
    return out.getvalue().splitlines()


@pytest.fixture()
def book_file(tmp_path):
    p = str(tmp_path / "book.npz")
    _book(GAMES).save(p)
    return p


def test_ucci_without_the_option_nothing_changes():
    script = "ucci\nisready\nposition startpos moves h2e2\nbanmoves h9g7\ngo nodes 40\nposition startpos\ngo nodes 24\nquit\n"
    plain, withbook = OracleSearcher(), BookSearcher()
    assert _session(script, plain) == _session(script, withbook) and withbook.calls == [] and plain.resets == withbook.resets == 2
    # set and unset again: the same
    s = BookSearcher()
    assert _session(script.replace("isready\n", "isready\nsetoption Book some file.npz\nsetoption Book none\n"), s) == _session(script, plain) and s.calls == []


def test_ucci_answers_from_the_book_without_a_search(book_file):
    s = BookSearcher()
    lines = _session("setoption Book %s\ngo nodes 40\nquit\n" % book_file, s)
    # the opening position: h2e2 / b2e2 are one entry of four games (+1, 0 from red's view, -1, 0), c3c4 one game: below BookMinGames 2
    L = O.labels()
    move = L[min(L.index("h2e2"), L.index("b2e2"))]
    assert lines == ["info string book games 4 wins 1 draws 2 losses 1", "info depth 1 score 0 nodes 0 time 0 pv %s" % move, "bestmove %s" % move, "bye"]
    assert s.resets == 0 and s.calls == [("book", book_file, 2, False)]
    s = BookSearcher()
    lines = _session("setoption Book %s\nsetoption BookMinGames 1\nsetoption BookSample true\nposition startpos moves c3c4\ngo\nquit\n" % book_file, s)
    assert lines == ["info string book games 1 wins 0 draws 0 losses 1", "info depth 1 score -1000 nodes 0 time 0 pv h9g7", "bestmove h9g7", "bye"]
    assert s.resets == 0 and s.calls == [("book", book_file, 1, True)]
    # not in the book, or too few games: the search
    for script in ("position startpos moves a0a1\ngo nodes 8\nquit\n", "position startpos moves c3c4\ngo nodes 8\nquit\n"):
        s = BookSearcher()
        lines = _session("setoption Book %s\n" % book_file + script, s)
        assert s.resets == 1 and len(s.calls) == 1 and not any(l.startswith("info string book") for l in lines)
        assert lines == _session(script, OracleSearcher())
    lines = _session("setoption BookSample maybe\nsetoption BookMinGames few\nquit\n", BookSearcher())
    assert len(lines) == 3 and all(l.startswith("info string setoption Book") for l in lines[:2])


def test_ucci_a_banned_book_move_falls_through(book_file):
    # after h2e2 the book holds h9g7 (games 0, 4 and, mirrored, 1) and b9c7 (game 2 alone)
    pos = "position startpos moves h2e2\n"
    s = BookSearcher()
    assert _session("setoption Book %s\n%sgo nodes 8\nquit\n" % (book_file, pos), s)[2] == "bestmove h9g7" and s.resets == 0
    s = BookSearcher()
    lines = _session("setoption Book %s\n%sbanmoves h9g7\ngo nodes 8\nquit\n" % (book_file, pos), s)
    assert s.resets == 1 and len(s.calls) == 1 and lines == _session(pos + "banmoves h9g7\ngo nodes 8\nquit\n", OracleSearcher())
    assert not lines[-2].startswith("bestmove h9g7")
    # with BookMinGames 1 the other book move is played instead, never the banned one
    s = BookSearcher()
    lines = _session("setoption Book %s\nsetoption BookMinGames 1\n%sbanmoves h9g7\ngo nodes 8\nquit\n" % (book_file, pos), s)
    assert lines[-2] == "bestmove b9c7" and s.resets == 0


def test_ucci_tablebase_and_mate_come_first(book_file):
    L = O.labels()
    s = BookSearcher(tb=(5, [L.index("c3c4")]))
    lines = _session("setoption Book %s\nsetoption Tablebase /tables\ngo\nquit\n" % book_file, s)
    assert lines[-2] == "bestmove c3c4" and [c[0] for c in s.calls] == ["tablebase"]
    s = BookSearcher(mate_line=(3, [L.index("a3a4")], 17))
    lines = _session("setoption Book %s\nsetoption Tablebase /tables\nsetoption MateSearch 3\ngo\nquit\n" % book_file, s)
    assert lines[-2] == "bestmove a3a4" and [c[0] for c in s.calls] == ["tablebase", "mate"]
    s = BookSearcher()
    lines = _session("setoption Book %s\nsetoption Tablebase /tables\nsetoption MateSearch 3\ngo\nquit\n" % book_file, s)
    assert lines[-2].startswith("bestmove ") and [c[0] for c in s.calls] == ["tablebase", "mate", "book"] and s.resets == 0


# ---- the kernels' metadata ---------------------------------------------------------------------------------------------------
def test_book_kernels_use_no_scratch(tmp_path):
    from cchess_zero_amd import build
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    out = str(tmp_path / "cz_book.s")
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(ROOT, "cchess_zero_amd", "csrc", "cz_book.hip")], check=True,
                   stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    seen = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read()):
        if "k_book_" in m.group(1):
            seen[m.group(1)] = int(m.group(2))
    assert len(seen) == 4 and all(v == 0 for v in seen.values()), seen      # keys, entries, probe, choose
