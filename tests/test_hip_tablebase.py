"""Endgame tablebases on the GPU (cz_tb_pass, cz_tb_probe, cz_tb_boards; cchess_zero_amd.tablebase.Tablebase):
  1. the built tables equal tests/tablebase_model.py's recorded ones bit for bit (tests/golden/tablebase_model.npz, which
     tests/test_tablebase_model_cpu.py holds to a fresh run of the model);
  2. independently of the model, Rules.mate(attacker="all") at 5 plies answers a table's wins within 5 plies, and nothing else;
  3. on a five-slot table nobody modelled (KR-KAB) every value is the pass rule applied to its children's FINAL values, the children
     made by the existing movegen_kingsafe -> successors path, and passes, wins, losses and crc32 are the host build's;
  4. probe and boards are inverse to each other, duplicates and foreign boards included;
  5. best / line play the model's principal line.
All tables are built once per module."""
import ctypes as C
import json

import numpy as np
import pytest

import tablebase_classes as TC
import tablebase_model as TM

pytestmark = pytest.mark.gpu

ILLEGAL, MISS = TM.ILLEGAL, TM.MISS
BUILT = ("K-K", "KP-K", "KR-K", "KN-K", "KC-K", "KN-KA", "KN-KB", "KR-KAA", "KP-KP")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def tb():
    from cchess_zero_amd.tablebase import Tablebase
    t = Tablebase()
    t.progress = []
    for s in BUILT[5:] + ("KR-K", "KC-K"):
        t.build(s, progress=lambda sig, d, got: t.progress.append((sig, d, got)))
    return t


@pytest.fixture(scope="module")
def golden():
    return TM.golden()


def _legal_positions(tb, torch, sig):
    v = tb.tables[sig]
    idx = (v != ILLEGAL).nonzero().flatten().to(torch.int32)
    boards, side = tb.boards(sig, idx)
    return idx, boards, side, v[idx.to(torch.int64)].to(torch.int32)


@pytest.mark.parametrize("sig", BUILT)
def test_tables_bit_for_bit(tb, golden, sig):
    """K-K's 162 entries are two full groups and a ragged one of 34; KN-KA needs 39 passes with captures both ways; KP-KP has
    wins for both colours and stops at the wrong place under "the first empty pass"."""
    values, passes = golden
    got = tb.tables[sig].cpu().numpy()
    st = tb.stats[sig]
    print("%s: %d passes (model %d), %s" % (sig, st["passes"], passes[sig], st))
    assert got.dtype == np.int16 and got.shape == values[sig].shape == (TM.entries(sig),)
    bad = np.nonzero(got != values[sig])[0]
    assert len(bad) == 0, (sig, len(bad), bad[:5], got[bad[:5]], values[sig][bad[:5]])
    assert st["passes"] == passes[sig]
    if sig == "KP-KP":
        side = np.arange(len(got)) & 1
        assert ((got > 0) & (got != TM.UNKNOWN) & (side == 0)).any() and ((got > 0) & (side == 1)).any()
        per_pass = [g for s, d, g in tb.progress if s == sig]
        first_empty = per_pass.index(0) + 1
        assert first_empty < st["passes"] and any(per_pass[first_empty:]), per_pass   # an empty pass with decided ones behind it
        assert st["wins"] == 13362 and st["longest_win"] == 21
    if sig == "KN-KA":
        assert st["passes"] >= 38 and st["longest_win"] == 37 and st["longest_loss"] == 38


@pytest.mark.parametrize("sig", ["KN-K", "KP-K"])
def test_against_the_mate_search(tb, torch, sig):
    """Rules.mate over all king-safe moves proves exactly the table's wins within its horizon, at their distance"""
    idx, boards, side, v = _legal_positions(tb, torch, sig)
    res = tb.rules.mate(boards, side, 5, attacker="all")
    v = v.cpu().numpy()
    near = (v > 0) & (v - 1 <= 5)
    assert near.sum() > 100 and (~near).sum() > 100
    assert np.array_equal(res["status"][near], np.ones(near.sum(), np.uint8)), np.nonzero(res["status"][near] != 1)[0][:5]
    assert np.array_equal(res["dist"][near], (v[near] - 1).astype(np.int16))
    assert not res["status"][~near].any(), (np.nonzero(res["status"][~near])[0][:5], np.unique(res["status"][~near]))


def test_fixpoint_on_a_table_nobody_modelled(tb, torch):
    """KR-KAB, 510 300 entries: every legal value is the pass rule on the children's final values; the children come from
    cz_tb_boards -> movegen_kingsafe -> successors -> probe, none of which the build uses.  And the table is the host build's."""
    sig = "KR-KAB"
    tb.build(sig)
    table = tb.tables[sig]
    assert table.shape == (510300,) and tb.stats[sig]["wins"] > 0 and tb.stats[sig]["losses"] > 0
    # the arithmetic is tests/tablebase_classes.py's, shared with tests/test_hip_tablebase_classes.py: every -1 entry, and no other, has
    # no king-safe move; every child is covered; the value is pass_rule of the children's values
    TC.check_fixpoint(tb, sig, (table != ILLEGAL).nonzero().flatten())
    # the ILLEGAL entries: two slots share a square (an empty board), or the mover can take the king, or the board is refused
    apart, overlapping = TC.check_illegal(tb, sig, (table == ILLEGAL).nonzero().flatten())
    assert apart > 0 and overlapping > 0
    # a fixpoint cannot see a build that stopped too early (deep wins left as draws are a fixpoint too): the host build's numbers
    got = TC.table_stats(table, tb.stats[sig]["passes"])
    print("%s: %s" % (sig, got))
    for k in ("passes", "wins", "losses", "crc32"):
        assert got[k] == TC.PINNED[sig][k], (k, got[k], TC.PINNED[sig][k])


def test_probe_and_boards(tb, torch):
    sig = "KR-KAA"
    table = tb.tables[sig]
    idx, boards, side, v = _legal_positions(tb, torch, sig)
    value, index = tb.probe_one(sig, boards, side, want_index=True)
    assert torch.equal(value.to(torch.int32), v)
    # among equal pieces the k-th in ascending square order stands on the k-th slot: the canonical index holds the same value
    assert torch.equal(table[index.to(torch.int64)].to(torch.int32), v)
    same = index == idx
    assert 0 < int(same.sum()) < idx.numel()
    b2, s2 = tb.boards(sig, index)
    assert torch.equal(b2, boards) and torch.equal(s2, side)
    value2, covered = tb.probe(boards, side)
    assert torch.equal(value2, value) and bool(covered.all())
    # against the model's rank, on a sample
    pick = torch.arange(0, idx.numel(), 997, device=idx.device)
    hb, hs, hi = boards[pick].cpu().numpy(), side[pick].cpu().numpy(), index[pick].cpu().numpy()
    assert [TM.rank(sig, b, s) for b, s in zip(hb, hs)] == list(hi)
    # boards of another signature (and the empty boards of its overlapping indices) miss
    kb, ks = tb.boards("KN-KA", torch.arange(0, 72900, 11, dtype=torch.int32))
    assert bool((tb.probe_one(sig, kb, ks) == MISS).all())
    # a mixed batch is grouped by its pieces; a signature that is not loaded, an empty board and a board of 32 pieces miss
    from cchess_zero_amd.rules import START_BOARD
    nb, ns = tb.boards("KN-KB", torch.arange(0, 102060, 13, dtype=torch.int32))
    rb, rs = boards[::29], side[::29]
    mixed = torch.cat([kb, rb, nb, torch.zeros((1, 90), dtype=torch.uint8, device=kb.device), torch.from_numpy(START_BOARD).to(kb.device).reshape(1, 90)])
    mside = torch.cat([ks, rs, ns, torch.zeros(2, dtype=torch.uint8, device=kb.device)])
    perm = torch.randperm(mixed.shape[0], generator=torch.Generator().manual_seed(5)).to(kb.device)
    mv_, mc = tb.probe(mixed[perm].contiguous(), mside[perm].contiguous())
    want = torch.cat([tb.probe_one("KN-KA", kb, ks), value[::29], tb.probe_one("KN-KB", nb, ns), torch.full((2,), MISS, dtype=torch.int16, device=kb.device)])
    assert torch.equal(mv_, want[perm]) and torch.equal(mc, (want[perm] != MISS) & (want[perm] != ILLEGAL))
    saved = tb.tables.pop("KN-KB")
    try:
        assert bool((tb.probe(nb, ns)[0] == MISS).all())
    finally:
        tb.tables["KN-KB"] = saved
    # G of 1, 64, 65 and 0
    for G in (1, 64, 65):
        gv, gi = tb.probe_one(sig, boards[:G].contiguous(), side[:G].contiguous(), want_index=True)
        assert torch.equal(gv, value[:G]) and torch.equal(gi, index[:G])
        gb, gs = tb.boards(sig, idx[:G])
        assert torch.equal(gb, boards[:G]) and torch.equal(gs, side[:G])
    assert tb.probe(boards[:0], side[:0])[0].shape == (0,) and tb.boards(sig, idx[:0])[0].shape == (0, 90)
    # boards at an address that is not 16-byte aligned: cz_tb_probe takes the byte path, cz_tb_boards refuses
    raw = torch.zeros(65 * 90 + 16, dtype=torch.uint8, device=kb.device)
    off = (2 - raw.data_ptr()) % 16
    un = raw[off:off + 65 * 90].view(65, 90)
    assert un.data_ptr() % 16 == 2
    un.copy_(boards[:65])
    out = torch.empty(65, dtype=torch.int16, device=kb.device)
    tb.ctx.call("cz_tb_probe", sig.encode(), table, un, side[:65].contiguous(), 65, out, None)
    assert torch.equal(out, value[:65])
    from cchess_zero_amd._lib import CchessHipError
    with pytest.raises(CchessHipError, match="cz_tb_boards: boards must be 16-byte aligned"):
        tb.ctx.call("cz_tb_boards", sig.encode(), idx[:65].contiguous(), 65, un, None)
    # an index outside the table is refused by Tablebase.boards; the kernel itself answers an empty board
    for bad in ([364500], [-1]):
        with pytest.raises(ValueError):
            tb.boards(sig, bad)
    eb = torch.full((3, 90), 7, dtype=torch.uint8, device=kb.device)
    es = torch.full((3,), 9, dtype=torch.uint8, device=kb.device)
    tb.ctx.call("cz_tb_boards", sig.encode(), torch.tensor([364500, -1, int(idx[0])], dtype=torch.int32, device=kb.device), 3, eb, es)
    assert not bool(eb[:2].any()) and not bool(es[:2].any()) and torch.equal(eb[2], boards[0])
    # bad arguments
    for call in (lambda: tb.ctx.call("cz_tb_probe", b"KR-KK", table, boards, side, 1, out, None), lambda: tb.ctx.call("cz_tb_pass", sig.encode(), table, None, 1, None),
                 lambda: tb.ctx.call("cz_tb_pass", sig.encode(), None, None, 0, None)):
        with pytest.raises(CchessHipError, match="cz_tb_"):
            call()
    n, s = C.c_longlong(), C.c_int()
    from cchess_zero_amd._lib import call as libcall
    libcall("cz_tb_entries", b"KRN-KR", C.byref(n), C.byref(s))
    assert (n.value, s.value) == (2 * 9 * 90 * 90 * 9 * 90, 5)
    with pytest.raises(CchessHipError, match="2\\^31"):
        libcall("cz_tb_entries", b"KRRNN-KRR", C.byref(n), C.byref(s))


class _G:
    def __init__(self, values):
        self.values = values


def test_best_and_line(tb, torch, golden, capsys, tmp_path):
    """From the longest KN-KA win: the line has exactly `plies` moves, every move is in its position's king-safe list, the values
    count down by one with alternating sign, the line ends in a position without a king-safe move, and it is the model's line,
    through the capture into KN-K where the model's has one."""
    from cchess_zero_amd import tablebase as TBM
    from cchess_zero_amd._lib import POS_NO_SAFE_MOVE
    import kingsafe_model as M
    from perft_model import make_move
    sig = "KN-KA"
    lg = tb.longest(sig)
    assert lg["plies"] == 37 and lg["index"] == int(np.argmax(golden[0][sig]))
    b, s = tb.boards(sig, [lg["index"]])
    board, side = b[0].cpu().numpy(), int(s[0])
    line = tb.line(board, side)
    model_line = TM.line({k: _G(v) for k, v in golden[0].items()}, board, side)
    assert len(line) == 37 and line == model_line
    bb, ss, sigs = board, side, []
    for k, m in enumerate(line):
        v = int(tb.probe(bb.reshape(1, 90), np.array([ss], np.uint8))[0][0])
        assert abs(v) - 1 == 37 - k and (v > 0) == (k % 2 == 0)
        assert m in [int(x) for x in M.kingsafe(bb, ss)[0]]
        sigs.append(TM.signature_of(bb))
        bb, ss = make_move(bb, m)[0], 1 - ss
    assert int(tb.rules.in_check(bb.reshape(1, 90), np.array([ss], np.uint8))[0]) & POS_NO_SAFE_MOVE
    assert int(tb.probe(bb.reshape(1, 90), np.array([ss], np.uint8))[0][0]) == -1
    assert sigs[0] == "KN-KA" and ("KN-K" in sigs) == any(make_move(*p)[1] for p in _walk(board, model_line))
    # best() on a batch: the first move of every line, a position without a move, an uncovered one
    from cchess_zero_amd.rules import START_BOARD
    batch = np.stack([board, bb, START_BOARD])
    label, value, nb, ns = tb.best(batch, np.array([side, ss, 0], np.uint8))
    assert label.cpu().tolist() == [line[0], -1, -1] and value.cpu().tolist() == [38, -1, MISS]
    assert np.array_equal(nb[0].cpu().numpy(), make_move(board, line[0])[0]) and int(ns[0]) == 1 - side
    # the command line gives the same line
    tb.save(str(tmp_path))
    sub = TBM.Tablebase(tb.rules)
    assert sub.load(str(tmp_path), ["KN-KA", "KN-K", "K-KA", "K-K"]) == ["KN-KA", "KN-K", "K-KA", "K-K"]
    assert torch.equal(sub.tables[sig], tb.tables[sig]) and sub.stats[sig] == tb.stats[sig]
    capsys.readouterr()
    TBM.main(["--probe", "--fen", lg["fen"], "--dir", str(tmp_path)], tb=sub)
    row = json.loads(capsys.readouterr().out)
    from cchess_zero_amd._lib import tables
    assert row["wdl"] == "win" and row["plies"] == 37 and row["signature"] == sig and row["pv"] == [tables()["labels"][m] for m in line]
    assert row["best"] == row["pv"][0] and row["pv"] == lg["pv"]
    # ... and so does the Analyzer, which leaves its search as it is
    from cchess_zero_amd import notation
    from cchess_zero_amd.analysis import Analyzer
    from cchess_zero_amd.net import PolicyValueNet
    an = Analyzer(PolicyValueNet(res_block_nums=1, seed=3), 16, 2)
    res = an.analyse([lg["fen"], notation.START_FEN], tablebase=sub)
    assert res[0]["tablebase"] == dict(wdl="win", plies=37, pv=row["pv"]) and res[1]["tablebase"] is None
    plain = an.analyse([lg["fen"], notation.START_FEN])
    assert all("tablebase" not in r for r in plain)
    for a, b in zip(res, plain):
        assert {k: v for k, v in a.items() if k != "tablebase"} == b


def _walk(board, line):
    b = board
    for m in line:
        yield b, m
        from perft_model import make_move
        b = make_move(b, m)[0]
