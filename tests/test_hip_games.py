"""cz_games_replay (csrc/cz_games.hip; games.GameReplayer) on the GPU against tests/games_model.py, byte for byte: the
reference's six self-play games plus the 130-game fault corpus of tests/games_cases.py (two full waves and a ragged one, stride
48, every status and every end_flags bit), at both rule levels — nothing larger.  The record buffer is pre-filled with 0xA5,
lies between sentinel records, and has a gap between two games' ranges that must stay 0xA5.  Then the host's length sort
(permuted rec_offset), the records through cz_records_expand, the replay of games.random_games against the ply-by-ply path that
made them, the argument checks of the C ABI, and main.py --pretrain in a child process."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import games_cases as GC
import games_model as GM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, GAP_AFTER, GAP = 0xA5, 40, 3


@pytest.fixture(scope="module")
def rp():
    from cchess_zero_amd.games import GameReplayer
    return GameReplayer()


@pytest.fixture(scope="module")
def corpus():
    """the six golden games in front of the fault corpus, as one batch of 136 games of stride 223"""
    c = GC.corpus()
    moves6, lens6, res6, _, _ = GM.golden_games()
    stride = moves6.shape[1]
    moves = np.full((6 + GC.G, stride), 0xFFFF, np.uint16)
    moves[:6] = moves6
    moves[6:, :GC.STRIDE] = c["moves"]
    return dict(boards=np.concatenate([np.tile(GM.start_board(), (6, 1)), c["boards"]]), side=np.concatenate([np.zeros(6, np.uint8), c["side"]]),
                moves=moves, lens=np.concatenate([lens6, c["lens"]]).astype(np.int32), results=np.concatenate([res6, c["results"]]).astype(np.int8))


def offsets_with_a_gap(lens, stride):
    ln = np.where((lens >= 0) & (lens <= stride), lens, 0).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(ln)[:-1]])
    off[GAP_AFTER + 1:] += GAP
    return off.astype(np.int32), int(ln.sum()) + GAP


_model = {}


def model(corpus, rules):
    if rules not in _model:
        off, total = offsets_with_a_gap(corpus["lens"], corpus["moves"].shape[1])
        _model[rules] = GM.replay(corpus["boards"], corpus["side"], corpus["moves"], corpus["lens"], corpus["results"], rules, off, total, FILL)
    return _model[rules]


def raw(rp, boards, side, moves, lens, results, rules, off, total, order=None, override=None):
    """cz_games_replay through the C ABI: the records between two sentinel records, every output pre-filled -> (rc, outputs)"""
    from cchess_zero_amd._lib import lib, _ptr
    G, stride = moves.shape
    sel = np.arange(G) if order is None else order
    alive = []                                       # the inputs live until the call has run: their addresses go in as numbers

    def t(a, dt):
        alive.append(None if a is None else rp.ctx.tensor(np.ascontiguousarray(a[sel]), dt))
        return alive[-1]
    buf = torch.full((total + 2, 608), FILL, dtype=torch.uint8, device=rp.dev)
    assert buf.data_ptr() % 16 == 0
    out = dict(valid=torch.full((G,), -7, dtype=torch.int32, device=rp.dev), status=torch.full((G,), 99, dtype=torch.uint8, device=rp.dev),
               end_flags=torch.full((G,), 99, dtype=torch.uint8, device=rp.dev), final_boards=torch.full((G, 90), 99, dtype=torch.uint8, device=rp.dev),
               final_side=torch.full((G,), 99, dtype=torch.uint8, device=rp.dev))
    args = dict(boards=_ptr(t(boards, torch.uint8)), side=_ptr(t(side, torch.uint8)), moves=_ptr(t(moves, torch.int16)), stride=stride,
                len=_ptr(t(lens, torch.int32)), result=_ptr(t(results, torch.int8)), G=G, rules=rules, off=_ptr(t(off, torch.int32)), total=total,
                records=C.c_void_p(buf.data_ptr() + 608), valid=_ptr(out["valid"]), status=_ptr(out["status"]), end_flags=_ptr(out["end_flags"]),
                final_boards=_ptr(out["final_boards"]), final_side=_ptr(out["final_side"]))
    args.update(override or {})
    rp.ctx.bind_stream()
    rc = lib().cz_games_replay(rp.ctx.h, *[args[k] for k in ("boards", "side", "moves", "stride", "len", "result", "G", "rules", "off", "total", "records",
                                                             "valid", "status", "end_flags", "final_boards", "final_side")])
    torch.cuda.synchronize()
    del alive
    h = buf.cpu().numpy()
    assert (h[0] == FILL).all() and (h[-1] == FILL).all(), "a sentinel record was written"
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if order is not None:
        inv = np.empty(G, np.int64)
        inv[order] = np.arange(G)
        res = {k: v[inv] for k, v in res.items()}
    res["records"] = h[1:-1]
    return rc, res


def hold(got, want):
    for k in ("valid", "status", "end_flags", "final_side", "final_boards", "records"):
        bad = np.nonzero(np.asarray(got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))[0]
        assert len(bad) == 0, (k, bad[:5], got[k][bad[:2]], want[k][bad[:2]])


@pytest.mark.parametrize("rules", [0, 1])
def test_the_device_against_the_model(rp, corpus, rules):
    want = model(corpus, rules)
    rc, got = raw(rp, corpus["boards"], corpus["side"], corpus["moves"], corpus["lens"], corpus["results"], rules, want["rec_offset"], want["total"])
    assert rc == 0
    hold(got, want)
    gap = int(want["rec_offset"][GAP_AFTER + 1]) - GAP
    assert (got["records"][gap:gap + GAP] == FILL).all() and set(want["status"].tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("rules", [0, 1])
def test_the_opening_position_when_no_start_is_given(rp, rules):
    moves, lens, results, _, _ = GM.golden_games()
    want = GM.replay(None, None, moves, lens, results, rules)
    rc, got = raw(rp, None, None, moves, lens, results, rules, want["rec_offset"], want["total"])
    assert rc == 0
    hold(got, want)


@pytest.mark.parametrize("rules", [0, 1])
def test_permuted_rec_offset_gives_the_records_in_input_order(rp, corpus, rules):
    """the host's length sort: the games in another order, their offsets with them"""
    want = model(corpus, rules)
    order = np.argsort(np.where((corpus["lens"] >= 0) & (corpus["lens"] <= 223), corpus["lens"], 0), kind="stable")[::-1].copy()
    assert (order != np.arange(len(order))).any()
    rc, got = raw(rp, corpus["boards"], corpus["side"], corpus["moves"], corpus["lens"], corpus["results"], rules, want["rec_offset"], want["total"],
                  order=order)
    assert rc == 0
    hold(got, want)


@pytest.mark.parametrize("rules", ["capture", "xiangqi"])
def test_the_replayer_sorts_drops_truncates_and_infers(rp, corpus, rules):
    from cchess_zero_amd import games as GG
    r = {"capture": 0, "xiangqi": 1}[rules]
    ok = (corpus["lens"] >= 0) & (corpus["lens"] <= 223)                  # a Game cannot say a length its moves do not have
    idx = np.nonzero(ok)[0]
    gs = GG.games_from_labels(corpus["moves"][idx], corpus["lens"][idx], corpus["results"][idx], corpus["boards"][idx], corpus["side"][idx])
    full = model(corpus, r)                                               # a game's answer does not depend on where its records go
    want = {k: full[k][idx] for k in ("valid", "status", "end_flags", "final_boards", "final_side")}
    want["per_game"] = [full["per_game"][i] for i in idx]
    for mode in ("drop", "truncate"):
        res = rp.replay(gs, rules=rules, on_illegal=mode, sort=(mode == "drop"))     # sorted by length, and in the order they came
        keep_game = (want["status"] == GM.OK) | (mode == "truncate")
        recs = [g["records"][:g["valid"]] for g, k in zip(want["per_game"], keep_game) if k]
        assert np.array_equal(res.records.cpu().numpy(), np.concatenate(recs))
        assert np.array_equal(res.game_of_record, np.repeat(np.nonzero(keep_game)[0], [len(x) for x in recs]).astype(np.int32))
        for k in ("valid", "status", "end_flags", "final_boards", "final_side"):
            assert np.array_equal(getattr(res, k), want[k]), k
        assert res.counts["ok"] == int((want["status"] == GM.OK).sum()) and res.counts["kept_plies"] == sum(len(x) for x in recs)
        assert res.counts["illegal"] + res.counts["after_end"] + res.counts["bad_board"] + res.counts["ok"] == len(gs) and res.counts["unknown_result"] == 0


def test_results_that_are_not_given(rp, corpus):
    """the position reached decides (five of the six golden games end with a king taken), and z is patched on the device"""
    from cchess_zero_amd import games as GG
    full = model(corpus, 0)
    gold = [g._replace(result=None) for g in GG.games_from_labels(corpus["moves"][:6], corpus["lens"][:6], corpus["results"][:6])]
    res = rp.replay(gold, rules="capture")
    won = [0, 1, 2, 4, 5]                                                 # game 3 is one ply long: nothing decides it
    assert res.results == [int(corpus["results"][g]) if g in won else None for g in range(6)]
    assert res.counts["unknown_result"] == 1 and res.counts["inferred_results"] == 5 and res.kept.tolist() == [g in won for g in range(6)]
    assert np.array_equal(res.records.cpu().numpy(), np.concatenate([full["per_game"][g]["records"] for g in won]))
    assert np.array_equal(res.game_of_record, np.repeat(won, corpus["lens"][won]).astype(np.int32))


def test_the_records_through_cz_records_expand(rp, corpus):
    """plain and mirrored, temperatures 1.0 and 0.25: to_dense(mirror_records(.)) of the model's records, pi one-hot at the played
    move's canonical label"""
    from cchess_zero_amd import games as GG
    from cchess_zero_amd._lib import tables
    from cchess_zero_amd.records import RecordExpander, mirror_records
    from cchess_zero_amd.selfplay import to_dense, unpack_records
    gs = GG.games_from_labels(corpus["moves"][:6], corpus["lens"][:6], corpus["results"][:6])
    res = rp.replay(gs, rules="capture")
    n = res.records.shape[0]
    assert n == 342
    ex = RecordExpander(ctx=rp.ctx)
    host = res.records.cpu().numpy()
    u = unpack_records(host)
    played = u["labels"][np.arange(n), u["visits"].argmax(axis=1)].astype(np.int64)
    t = tables()
    for flags in (np.zeros(n, np.uint8), np.ones(n, np.uint8), (np.arange(n) % 3 == 0).astype(np.uint8)):
        lab = np.where(flags != 0, t["mirror"][played], played)
        lab = np.where(u["side"] != 0, t["unflip"][lab], lab)
        for temperature in (1.0, 0.25):
            planes, pi, z = ex.expand(res.records, flags, temperature)
            wp, wpi, wz = to_dense(mirror_records(host, flags), temperature, exact=True)
            assert np.array_equal(planes.cpu().numpy(), wp) and np.array_equal(z.cpu().numpy(), wz)
            pi = pi.cpu().numpy()
            assert np.array_equal(pi, wpi.astype(np.float32))
            assert (pi[np.arange(n), lab] == 1.0).all() and (pi.sum(axis=1) == 1.0).all()


@pytest.mark.parametrize("rules", ["capture", "xiangqi"])
def test_against_random_games(rp, rules):
    """random_games builds its games ply by ply out of the stand-alone calls; their replay is all CZ_GAME_OK and reaches exactly
    the boards that path reached — also with the recorded moves fed back through that path (the yardstick of the measurement)"""
    from cchess_zero_amd import games as GG
    from cchess_zero_amd.rules import Rules
    R = Rules(ctx=rp.ctx)
    rg = GG.random_games(rules, 130, 5, 48, engine_rules=R)
    assert rg["lens"].max() > 30 and len(set(rg["lens"].tolist())) > 20 and (rg["moves"] != 0xFFFF).sum() == rg["lens"].sum()
    res = rp.replay(GG.games_from_labels(rg["moves"], rg["lens"], np.zeros(130, np.int8)), rules=rules)
    assert (res.status == GM.OK).all() and np.array_equal(res.valid, rg["lens"])
    assert np.array_equal(res.final_boards, rg["final_boards"]) and np.array_equal(res.final_side, rg["final_side"])
    assert res.records.shape[0] == int(rg["lens"].sum())
    v, fb, fs = GG.ply_by_ply_replay(rules, rg["moves"], rg["lens"], engine_rules=R)
    assert np.array_equal(v.cpu().numpy(), rg["lens"]) and np.array_equal(fb.cpu().numpy(), rg["final_boards"]) and np.array_equal(fs.cpu().numpy(), rg["final_side"])


def test_arguments_through_the_c_abi(rp):
    from cchess_zero_amd._lib import lib
    moves, lens, results, _, _ = GM.golden_games()
    want = GM.replay(None, None, moves, lens, results, 0)
    a = (None, None, moves, lens, results, 0, want["rec_offset"], want["total"])
    untouched = lambda g: (g["records"] == FILL).all() and (g["valid"] == -7).all() and (g["status"] == 99).all() and (g["final_boards"] == 99).all()
    rc, got = raw(rp, *a, override=dict(G=0))
    assert rc == 0 and untouched(got)                # G == 0: no launch
    null = C.c_void_p(None)
    aligned = torch.empty(608 * 400 + 64, dtype=torch.uint8, device=rp.dev)
    for bad in (dict(moves=null), dict(len=null), dict(result=null), dict(off=null), dict(valid=null), dict(status=null), dict(end_flags=null),
                dict(stride=-1), dict(rules=2), dict(rules=-1), dict(G=-1), dict(total=-1), dict(final_side=null),
                dict(records=C.c_void_p(aligned.data_ptr() + 8))):
        rc, got = raw(rp, *a, override=bad)
        assert rc == -1 and b"cz_games_replay" in lib().cz_last_error(), bad
        assert untouched(got), bad                   # a refused call writes nothing
    rc, got = raw(rp, *a, override=dict(final_boards=null, final_side=null))     # both may be left out
    assert rc == 0 and np.array_equal(got["records"], want["records"]) and (got["final_boards"] == 99).all()
    rc, got = raw(rp, *a, override=dict(records=null))                            # and so may the records
    assert rc == 0 and (got["records"] == FILL).all() and np.array_equal(got["valid"], want["valid"]) and np.array_equal(got["final_boards"], want["final_boards"])


def test_main_pretrain(tmp_path):
    """main.py --pretrain on the six golden games, in a fresh child process: a `pretrain` line with the model's counts, a training
    loss that goes down (it overfits 342 one-hot samples with fixed seeds: only the direction is asserted), and no such line
    without the flag."""
    from cchess_zero_amd import games as GG
    moves, lens, results, _, _ = GM.golden_games()
    path = str(tmp_path / "six.pgn")
    open(path, "w").write(GG.write_games(GG.games_from_labels(moves, lens, results), pgn=True))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, os.path.join(ROOT, "main.py"), "--mode", "train", "--games", "4", "--train_playout", "8", "--max_batches", "1",
            "--res_block_nums", "1"]
    p = subprocess.run(base + ["--pretrain", path, "--pretrain_steps", "20"], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=600,
                       stdin=subprocess.DEVNULL)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("pretrain: ")]
    assert len(lines) == 1, p.stdout[-3000:]
    d = json.loads(lines[0][len("pretrain: "):])
    m = GM.replay(None, None, moves, lens, results, 0)
    assert d["games"] == 6 and d["plies"] == 342 and d["ok"] == int((m["status"] == 0).sum()) == 6 and d["kept_plies"] == 342 and d["rules"] == "capture"
    assert d["illegal"] == d["after_end"] == d["bad_board"] == d["bad_len"] == d["unknown_result"] == 0
    assert d["red_king_gone"] + d["black_king_gone"] == 5 and d["steps"] == 20 and d["holdout_games"] == 1
    assert d["train_records"] + d["holdout_records"] == 342 and 0.0 <= d["top1"] <= 1.0 and d["logloss"] > 0
    print("pretrain losses:", d["losses"])
    assert len(d["losses"]) == 20 and np.mean(d["losses"][-5:]) < np.mean(d["losses"][:5]), d["losses"]
    assert p.stdout.index("pretrain: ") < p.stdout.index("batch i:")       # before the first self-play batch
    q = subprocess.run(base, capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=600, stdin=subprocess.DEVNULL)
    assert q.returncode == 0 and "pretrain" not in q.stdout, (q.stdout[-1500:], q.stderr[-3000:])
