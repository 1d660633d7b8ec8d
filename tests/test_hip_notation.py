"""cz_games_read (csrc/cz_notation.hip; games.GameReplayer with games of tokens) on the GPU against tests/notation_model.py, byte
for byte: the 131-game corpus of tests/notation_cases.py (two full waves and a ragged one; the reference's six games written by
the writer, label tokens among text tokens, every form of the notation, both ways to be ambiguous, garbage, every status) at
both rule levels, every output pre-filled with a sentinel and the records between two sentinel records.  Then label tokens alone
against cz_games_replay on its own fault corpus, the replayer on WXF-written copies of random games, the argument checks of the
C ABI, and the command line on a small file in Chinese notation."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import games_cases as GC
import notation_cases as NC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
KEYS = ("valid", "status", "end_flags", "final_side", "final_boards", "labels_out", "records")
NAMES = ("boards", "side", "tokens", "stride", "len", "result", "G", "rules", "off", "total", "records", "valid", "status", "end_flags", "final_boards",
         "final_side", "labels_out")


@pytest.fixture(scope="module")
def rp():
    from cchess_zero_amd.games import GameReplayer
    return GameReplayer()


def offsets_of(lens, stride):
    ln = np.where((lens >= 0) & (lens <= stride), lens, 0).astype(np.int64)
    return np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int32), int(ln.sum())


def raw(rp, boards, side, tokens, lens, results, rules, override=None, entry="cz_games_read"):
    """cz_games_read (or, tokens being uint16 labels, cz_games_replay) through the C ABI: the records between two sentinel records,
    every output pre-filled -> (rc, outputs)"""
    from cchess_zero_amd._lib import lib, _ptr
    G, stride = tokens.shape
    off, total = offsets_of(lens, stride)
    alive = []                                       # the inputs live until the call has run: their addresses go in as numbers

    def t(a, dt):
        alive.append(None if a is None else rp.ctx.tensor(np.ascontiguousarray(a), dt))
        return alive[-1]
    buf = torch.full((total + 2, 608), FILL, dtype=torch.uint8, device=rp.dev)
    out = dict(valid=torch.full((G,), -7, dtype=torch.int32, device=rp.dev), status=torch.full((G,), 99, dtype=torch.uint8, device=rp.dev),
               end_flags=torch.full((G,), 99, dtype=torch.uint8, device=rp.dev), final_boards=torch.full((G, 90), 99, dtype=torch.uint8, device=rp.dev),
               final_side=torch.full((G,), 99, dtype=torch.uint8, device=rp.dev),
               labels_out=torch.full((G, stride), 0x5A5A, dtype=torch.int16, device=rp.dev))
    args = dict(boards=_ptr(t(boards, torch.uint8)), side=_ptr(t(side, torch.uint8)),
                tokens=_ptr(t(tokens, torch.int32 if tokens.dtype == np.uint32 else torch.int16)), stride=stride,
                len=_ptr(t(lens, torch.int32)), result=_ptr(t(results, torch.int8)), G=G, rules=rules, off=_ptr(t(off, torch.int32)), total=total,
                records=C.c_void_p(buf.data_ptr() + 608), valid=_ptr(out["valid"]), status=_ptr(out["status"]), end_flags=_ptr(out["end_flags"]),
                final_boards=_ptr(out["final_boards"]), final_side=_ptr(out["final_side"]), labels_out=_ptr(out["labels_out"]))
    args.update(override or {})
    rp.ctx.bind_stream()
    names = NAMES if entry == "cz_games_read" else NAMES[:-1]
    rc = getattr(lib(), entry)(rp.ctx.h, *[args[k] for k in names])
    torch.cuda.synchronize()
    del alive
    h = buf.cpu().numpy()
    assert (h[0] == FILL).all() and (h[-1] == FILL).all(), "a sentinel record was written"
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["labels_out"] = res["labels_out"].view(np.uint16)
    res["records"] = h[1:-1]
    return rc, res


def hold(got, want, keys=KEYS):
    for k in keys:
        bad = np.nonzero(np.asarray(got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[0]
        assert len(bad) == 0, (k, bad[:5], got[k][bad[:2]], want[k][bad[:2]])


@pytest.mark.parametrize("rules", [0, 1])
def test_the_device_against_the_model(rp, rules):
    c = NC.corpus()
    rc, got = raw(rp, c["boards"], c["side"], c["tokens"], c["lens"], c["results"], rules)
    assert rc == 0
    hold(got, c["model"][rules])
    assert set(got["status"].tolist()) == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("rules", [0, 1])
def test_label_tokens_alone_equal_the_label_replay(rp, rules):
    c = GC.corpus()
    rc0, want = raw(rp, c["boards"], c["side"], c["moves"], c["lens"], c["results"], rules, entry="cz_games_replay")
    rc1, got = raw(rp, c["boards"], c["side"], c["moves"].astype(np.uint32), c["lens"], c["results"], rules)
    assert rc0 == 0 and rc1 == 0
    hold(got, want, [k for k in KEYS if k != "labels_out"])
    hold(got, c["model"][rules], [k for k in KEYS if k != "labels_out"])
    assert np.array_equal(got["labels_out"], np.where(np.arange(GC.STRIDE)[None, :] < got["valid"][:, None], c["moves"], 0xFFFF))


@pytest.mark.parametrize("rules", ["capture", "xiangqi"])
def test_the_replayer_on_wxf_copies_of_random_games(rp, rules):
    """200 random games written in WXF from their own replay, parsed back to tokens and replayed: the records of the ICCS
    originals, and the labels they were made of"""
    from cchess_zero_amd import games as GG
    from cchess_zero_amd.rules import Rules
    rg = GG.random_games(rules, 200, 7, 60, engine_rules=Rules(ctx=rp.ctx))
    gs = GG.games_from_labels(rg["moves"], rg["lens"], np.zeros(200, np.int8))
    a = rp.replay(gs, rules=rules)
    assert (a.status == 0).all() and a.counts["ambiguous"] == 0
    text = GG.write_games(gs, pgn=True, notation="wxf", replay=a)
    assert text.count('[Format "WXF"]') == 200
    back = GG.parse_games(text, notations=("wxf",))
    assert len(back) == 200 and back.skipped == () and all(g.tokens is not None and g.labels == () for g in back)
    b = rp.replay(back, rules=rules)
    assert (b.status == 0).all() and np.array_equal(b.valid, rg["lens"]) and torch.equal(a.records, b.records)
    assert np.array_equal(b.labels, a.labels) and np.array_equal(b.labels, rg["moves"][:, :b.labels.shape[1]])
    assert np.array_equal(b.final_boards, rg["final_boards"]) and np.array_equal(b.game_of_record, a.game_of_record)
    mixed = rp.replay(list(back[:100]) + gs[100:], rules=rules, sort=True)      # label games and token games in one launch, sorted
    assert torch.equal(mixed.records, a.records) and np.array_equal(mixed.labels, a.labels)


def test_arguments_through_the_c_abi(rp):
    from cchess_zero_amd._lib import lib
    c = NC.corpus()
    sel = np.arange(6, 40)
    a = (c["boards"][sel], c["side"][sel], np.ascontiguousarray(c["tokens"][sel, :40]), c["lens"][sel], c["results"][sel], 0)
    want = {k: v[sel] for k, v in c["model"][0].items() if k in ("valid", "status", "final_boards")}
    untouched = lambda g: ((g["records"] == FILL).all() and (g["valid"] == -7).all() and (g["status"] == 99).all() and (g["final_boards"] == 99).all()
                           and (g["labels_out"] == 0x5A5A).all())
    rc, got = raw(rp, *a, override=dict(G=0))
    assert rc == 0 and untouched(got)                # G == 0: no launch
    null = C.c_void_p(None)
    aligned = torch.empty(608 * 2000 + 64, dtype=torch.uint8, device=rp.dev)
    odd = torch.empty(34 * 40 * 4 + 8, dtype=torch.uint8, device=rp.dev)
    for bad in (dict(tokens=null), dict(len=null), dict(result=null), dict(off=null), dict(valid=null), dict(status=null), dict(end_flags=null),
                dict(stride=-1), dict(stride=65536), dict(rules=2), dict(rules=-1), dict(G=-1), dict(total=-1), dict(final_side=null),
                dict(records=C.c_void_p(aligned.data_ptr() + 8)), dict(tokens=C.c_void_p(odd.data_ptr() + 2)),
                dict(labels_out=C.c_void_p(odd.data_ptr() + 1))):
        rc, got = raw(rp, *a, override=bad)
        assert rc == -1 and b"cz_games_read" in lib().cz_last_error(), bad
        assert untouched(got), bad                   # a refused call writes nothing
    rc, got = raw(rp, *a, override=dict(labels_out=null, final_boards=null, final_side=null, records=null))     # all four may be left out
    assert rc == 0 and (got["labels_out"] == 0x5A5A).all() and (got["records"] == FILL).all() and np.array_equal(got["valid"], want["valid"])
    assert np.array_equal(got["status"], want["status"])


def test_the_command_line_reads_chinese_and_writes_it_back(tmp_path):
    """python -m cchess_zero_amd.games --notation any --write-pgn on a small file in Chinese notation, in a child process; what it
    wrote reads back to the same tokens"""
    from cchess_zero_amd import games as GG
    src, dst = str(tmp_path / "zh.pgn"), str(tmp_path / "out.pgn")
    text = ('[Event "an opening"]\n[Format "Chinese"]\n[Result "1-0"]\n\n1. 炮二平五 馬8進7 2. 馬二進三 車9平8\n3. 車一平二 卒7進1 4. 車二進六 馬2進3 1-0\n\n'
            '[Result "0-1"]\n\n1. 炮二平五 炮８平５ 2. 傌二进三 马8进7 0-1\n\n'
            '[Result "1-0"]\n\n1. C2=5 H8+7 2. H2+3 1-0\n\n'
            '[Result "1-0"]\n\n1. h2e2 h9g7 1-0\n\n'
            '[Result "1-0"]\n\n1. 炮二平五 h9g7 1-0\n')                       # the last one mixes two notations
    open(src, "w", encoding="utf-8").write(text)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "cchess_zero_amd.games", "--in", src, "--notation", "any", "--rules", "xiangqi", "--write-pgn", dst,
                        "--write-notation", "chinese"], capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300, stdin=subprocess.DEVNULL)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["games"] == 4 and d["plies"] == 8 + 4 + 3 + 2 and d["kept_games"] == 4 and d["status"]["ok"] == 4 and d["status"]["ambiguous"] == 0
    assert len(d["skipped_blocks"]) == 1 and "h9g7" in d["skipped_blocks"][0][1]
    out = open(dst, encoding="utf-8").read()
    assert out.count('[Format "Chinese"]') == 4 and "1. 炮二平五 馬8進7 2. 馬二進三 車9平8 3. 車一平二 卒7進1 4. 車二進六 馬2進3 1-0" in out
    back = GG.parse_games(out, notations=GG.NOTATIONS)
    first = GG.parse_games(text, notations=GG.NOTATIONS)
    l2i = {s: i for i, s in enumerate(__import__("oracle.oracle", fromlist=["x"]).labels())}
    assert [g.tokens for g in back[:3]] == [g.tokens for g in first[:3]] and back[3].tokens == (GG.wxf_token("C2=5"), GG.wxf_token("H8+7"))
    assert first[3].labels == (l2i["h2e2"], l2i["h9g7"]) and back[0].tags == (("Event", "an opening"),) and [g.result for g in back] == [1, -1, 1, 1]
