"""The left-right mirror of the move vocabulary and of packed self-play records, and the mirror / expand arguments of
train.policy_update, on the CPU: the table (cz_mirror_table) against the label strings and against the C oracle's move
generator on every golden position; records.mirror_records against the reference's own pi of tests/golden/selfplay.npz; the
random draws of policy_update (the parent's index draw unchanged, one coin per drawn index after it, the same on every rank);
and the code-object metadata of the expansion kernel (no scratch)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import records_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tab():
    import __graft_entry__
    __graft_entry__.build_hip_only()
    from cchess_zero_amd._lib import tables
    return tables()


@pytest.fixture(scope="module")
def golden(tab):
    return RC.golden()


def test_mirror_table_is_the_file_mirror_of_the_labels(tab):
    mirror, unflip, labels = tab["mirror"].astype(np.int64), tab["unflip"].astype(np.int64), tab["labels"]
    assert mirror.shape == (2086,) and np.array_equal(np.sort(mirror), np.arange(2086))      # a permutation
    assert np.array_equal(mirror[mirror], np.arange(2086))                                  # an involution
    fixed = np.nonzero(mirror == np.arange(2086))[0]
    assert len(fixed) == 90 and all(labels[i][0] == "e" and labels[i][2] == "e" for i in fixed)
    assert np.array_equal(mirror[unflip], unflip[mirror])
    assert [labels[i] for i in mirror] == [RC.file_mirror(s) for s in labels]


def test_mirrored_boards_have_the_mirrored_legal_moves(tab, rules_golden):
    from oracle import oracle as O
    mirror = tab["mirror"].astype(np.int64)
    boards, side = rules_golden["boards"], rules_golden["side"]
    assert len(boards) == 4381
    mismatches, same_order, self_mirror = 0, 0, 0
    for b, s in zip(boards, side):
        mb = np.ascontiguousarray(b.reshape(10, 9)[:, ::-1]).reshape(90)
        want = mirror[O.legal_moves(b, int(s)).astype(np.int64)]
        got = O.legal_moves(mb, int(s)).astype(np.int64)
        mismatches += set(got.tolist()) != set(want.tolist()) or len(got) != len(want)
        same_order += np.array_equal(got, want)
        self_mirror += np.array_equal(mb, b)
    assert mismatches == 0
    print("mirrored move lists: %d of %d in generation order, %d boards are their own mirror image" % (same_order, len(boards), self_mirror))
    assert same_order < len(boards)   # generation order is NOT preserved: a mirrored record keeps the original child order
    assert self_mirror > 0            # ... and a board that is its own mirror image is among the cases


def test_mirror_records_against_the_reference_pi(tab, golden):
    from cchess_zero_amd.records import mirror_records
    from cchess_zero_amd.selfplay import canonical_planes, to_dense, unpack_records
    rec, pi_ref = golden
    assert rec.shape == (342, 608)
    m = mirror_records(rec)
    assert m.dtype == np.uint8 and m.shape == rec.shape and not np.array_equal(m, rec)
    assert np.array_equal(mirror_records(m), rec)                                            # an involution
    u, um = unpack_records(rec), unpack_records(m)
    for k in ("side", "counts", "z", "flags", "ply", "visits"):
        assert np.array_equal(u[k], um[k]), k
    assert np.array_equal(um["boards"].reshape(-1, 10, 9), u["boards"].reshape(-1, 10, 9)[:, :, ::-1])
    live = np.arange(128)[None, :] < u["counts"][:, None]
    assert np.array_equal(um["labels"][~live], u["labels"][~live])
    assert np.array_equal(um["labels"][live], tab["mirror"].astype(np.uint16)[u["labels"][live]])
    # the unmirrored expansion is the reference's tuple; the mirrored one is its pi permuted on CANONICAL labels, exactly
    assert np.array_equal(to_dense(rec)[1], pi_ref)
    planes, pi, z = to_dense(m)
    want = np.zeros_like(pi_ref)
    want[:, tab["mirror"].astype(np.int64)] = pi_ref
    assert pi.dtype == np.float64 and np.array_equal(pi, want)
    assert np.array_equal(planes, canonical_planes(um["boards"], um["side"])) and np.array_equal(z, u["z"].astype(np.float32))
    # per-record flags: only the flagged records change
    flags = (np.arange(len(rec)) % 3 == 1)
    part = mirror_records(rec, flags)
    assert np.array_equal(part[flags], m[flags]) and np.array_equal(part[~flags], rec[~flags])
    assert np.array_equal(mirror_records(rec, np.zeros(len(rec), np.uint8)), rec)


class _FakeNet:
    """policy_update's net surface without a network, in the style of tests/test_train.py"""
    module = None

    def __init__(self, step):
        self.global_step = step

    def forward(self, sb):
        n = len(sb)
        return np.zeros((n, 2086), np.float32), np.zeros((n, 1), np.float32)

    def train_step(self, sb, pb, wb, lr):
        self.global_step += 1
        return 0.5, 1.25, self.global_step

    def save(self, step):
        pass


def _update(monkeypatch, buf, seed, step, mirror, world=1, rank=0, batch=16):
    """one policy_update with a host expander that records what it is handed -> (records [k, 608], flags or None, info)"""
    from cchess_zero_amd import train
    from cchess_zero_amd.records import mirror_records
    from cchess_zero_amd.selfplay import to_dense
    seen = {}

    def expand(rec, flags, temperature):
        seen["rec"], seen["flags"] = rec.copy(), None if flags is None else np.array(flags)
        return to_dense(rec if flags is None else mirror_records(rec, flags), temperature)
    if world > 1:   # the rank arithmetic without a process group
        monkeypatch.setattr(train, "_dist_on", lambda: True)
        monkeypatch.setattr(train.dist, "get_world_size", lambda: world)
        monkeypatch.setattr(train.dist, "get_rank", lambda: rank)
        monkeypatch.setattr(train.dist, "get_backend", lambda: "gloo")
        monkeypatch.setattr(train.dist, "all_reduce", lambda t: None)
        monkeypatch.setattr(train, "broadcast_weights", lambda module, src=0: None)
    _, info = train.policy_update(_FakeNet(step), buf, batch, 1, 0.001, 1.0, 0.025, seed=seed, log=lambda *a: None, mirror=mirror,
                                  expand=expand)
    monkeypatch.undo()
    return seen["rec"], seen["flags"], info


def test_policy_update_draws(tab, golden, monkeypatch):
    rec = golden[0]
    buf = [r for r in rec]
    seed, step = 20260925, 7
    idx = random.Random((seed << 32) ^ step).sample(range(len(buf)), 16)    # the parent commit's draw
    got, flags, info = _update(monkeypatch, buf, seed, step, mirror=False)
    assert flags is None and np.array_equal(got, rec[idx]) and info["mirrored"] == 0
    # mirror=True: the same indices, then one coin per index from the same generator
    got1, flags1, info1 = _update(monkeypatch, buf, seed, step, mirror=True)
    rng = random.Random((seed << 32) ^ step)
    assert rng.sample(range(len(buf)), 16) == idx
    coins = np.array([rng.getrandbits(1) for _ in idx], np.uint8)
    assert np.array_equal(got1, rec[idx]) and flags1.dtype == np.uint8 and np.array_equal(flags1, coins)
    assert info1["mirrored"] == int(coins.sum()) and 0 < coins.sum() < 16
    # a function of (seed, global step) alone: another buffer of the same length, the same coins; another step or seed, others
    assert np.array_equal(_update(monkeypatch, buf[::-1], seed, step, mirror=True)[1], coins)
    assert not np.array_equal(_update(monkeypatch, buf, seed, step + 1, mirror=True)[1], coins)
    assert not np.array_equal(_update(monkeypatch, buf, seed + 1, step, mirror=True)[1], coins)
    # every rank decides alike: the rank slices of world 2 and 8 interleave to the world-1 batch
    for world in (2, 8):
        recs, fl, total = np.zeros_like(got1), np.zeros_like(coins), 0
        for rank in range(world):
            r, f, inf = _update(monkeypatch, buf, seed, step, mirror=True, world=world, rank=rank)
            assert len(r) == len(f) == 16 // world and inf["mirrored"] == int(f.sum())
            recs[rank::world], fl[rank::world] = r, f
            total += inf["mirrored"]
        assert np.array_equal(recs, got1) and np.array_equal(fl, coins) and total == int(coins.sum())


def test_policy_update_host_mirror_path(tab, golden, monkeypatch):
    """mirror=True without an expander: the host path runs on mirror_records of the drawn records"""
    from cchess_zero_amd import train
    from cchess_zero_amd.records import mirror_records
    from cchess_zero_amd.selfplay import to_dense
    rec = golden[0]
    seed, step = 3, 11
    rng = random.Random((seed << 32) ^ step)
    idx = rng.sample(range(len(rec)), 12)
    coins = np.array([rng.getrandbits(1) for _ in idx], np.uint8)
    want = to_dense(mirror_records(rec[idx], coins), 0.5)
    seen = {}

    class Net(_FakeNet):
        def train_step(self, sb, pb, wb, lr):
            seen["batch"] = (np.array(sb), np.array(pb), np.array(wb))
            return _FakeNet.train_step(self, sb, pb, wb, lr)
    _, info = train.policy_update(Net(step), [r for r in rec], 12, 1, 0.001, 1.0, 0.025, seed=seed, log=lambda *a: None, temperature=0.5,
                                  mirror=True)
    assert info["mirrored"] == int(coins.sum())
    assert np.array_equal(seen["batch"][0], want[0]) and np.array_equal(seen["batch"][1], want[1])
    assert np.array_equal(seen["batch"][2][:, 0], want[2])
    with pytest.raises(ValueError):   # dense tuples cannot be mirrored
        train.policy_update(_FakeNet(0), [(want[0][0], want[1][0], 0.0)] * 4, 2, 1, 0.001, 1.0, 0.025, log=lambda *a: None, mirror=True)


def test_trainer_takes_tensors_as_they_are():
    from cchess_zero_amd.net import PolicyValueModule
    from cchess_zero_amd.train import Trainer
    tr = Trainer(PolicyValueModule(1, seed=0))
    g = torch.Generator().manual_seed(1)
    x, pi, z = torch.rand((3, 9, 10, 14), generator=g), torch.rand((3, 2086), generator=g), torch.tensor([1.0, -1.0, 0.0])
    tx, tpi, tz = tr._tensors(x, pi, z)
    assert tx.shape == (3, 14, 9, 10) and torch.equal(tx, x.permute(0, 3, 1, 2)) and torch.equal(tpi, pi) and torch.equal(tz, z.reshape(3, 1))
    assert tpi.data_ptr() == pi.data_ptr()   # no copy through numpy
    ax, api, az = tr._tensors(x.numpy(), list(pi.numpy()), z.numpy().reshape(3, 1))   # arrays and lists as before
    assert torch.equal(ax, tx) and torch.equal(api, tpi) and torch.equal(az, tz)


def test_expand_kernel_uses_no_scratch(tmp_path):
    from cchess_zero_amd import build
    csrc = os.path.join(ROOT, "cchess_zero_amd", "csrc")
    flags = [f for f in build.FLAGS if f not in ("-shared", "-fPIC")]
    out = str(tmp_path / "cz_records.s")
    subprocess.run([build.hipcc()] + flags + ["--offload-device-only", "-S", "-o", out, os.path.join(csrc, "cz_records.hip")], check=True,
                   stdin=subprocess.DEVNULL, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert "cz_records.hip" in build.SOURCES
    found = [(m.group(1), int(m.group(2))) for m in
             re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", open(out).read()) if "k_records_expand" in m.group(1)]
    assert found and all(size == 0 for _, size in found), found
