"""SURVEY §8 row f1 — the training step and the policy update (policy_value_network.py:77-126,186-199; main.py:1157-1204).

  * Trainer.train_step (cchess_zero_amd/train.py, fp32 torch) against an independent float64 restatement of the
    reference graph's loss and optimiser written from the TF semantics (NHWC activations, HWIO kernels, batch-statistic
    BatchNorm without affine terms, softmax cross-entropy + MSE + 1e-4 * sum(w^2)/2 over ALL trainables, global-norm clip
    100, Nesterov momentum 0.9 applied the way tf.train.MomentumOptimizer does): loss, gradient norm and the weight
    updates of two consecutive steps (the second exercises the momentum slots).
  * policy_update under torch.distributed (gloo, world 2, CPU): every rank takes the same number of steps (the KL that
    drives the early stop is all-reduced), ends with bit-identical weights and the same lr_multiplier; rank 0 alone saves.
"""
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(n, seed):
    import nethelpers as H
    rng = np.random.default_rng(seed)
    x = H.positions(n, seed)
    pi = rng.random((n, 2086)) ** 8
    pi = (pi / pi.sum(axis=1, keepdims=True)).astype(np.float32)
    z = rng.choice([-1.0, 0.0, 1.0], size=(n, 1)).astype(np.float32)
    return x, pi, z


def _tf_loss64(w, x, pi, z, blocks, c_l2=1e-4):
    """The reference graph in float64, TF layout (policy_value_network.py:45-92), training mode."""
    idx = [0]

    def convbn(h, relu):
        i = idx[0]
        idx[0] += 1
        k = w["conv%d/kernel" % i]                                      # HWIO
        y = F.conv2d(h.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), w["conv%d/bias" % i], padding=k.shape[0] // 2).permute(0, 2, 3, 1)
        m = y.mean(dim=(0, 1, 2))
        v = ((y - m) ** 2).mean(dim=(0, 1, 2))                            # fused batch norm normalises with the biased variance
        y = (y - m) / torch.sqrt(v + 1e-5)
        return torch.relu(y) if relu else y
    h = convbn(x, True)
    for _ in range(blocks):
        t = convbn(h, True)
        t = convbn(t, False)
        h = torch.relu(h + t)
    p = convbn(h, True).reshape(x.shape[0], 180)
    logits = p @ w["policy_fc/weights"] + w["policy_fc/biases"]
    v = convbn(h, True).reshape(x.shape[0], 90)
    v = torch.relu(v @ w["value_fc1/weights"] + w["value_fc1/biases"])
    v = torch.tanh(v @ w["value_fc2/weights"] + w["value_fc2/biases"])
    policy_loss = (-(pi * torch.log_softmax(logits, dim=1)).sum(dim=1)).mean()
    value_loss = ((z - v) ** 2).mean()
    trainables = [t for k, t in w.items() if not k.startswith("bn")]
    l2 = c_l2 * sum((t * t).sum() / 2 for t in trainables)
    return value_loss + policy_loss + l2, trainables


def _run_restatement(w0, batches, lr, blocks, momentum=0.9, clip=100.0, accum0=None):
    w = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=not k.startswith("bn")) for k, v in w0.items()}
    names = [k for k in w if not k.startswith("bn")]
    accum = {k: (torch.zeros_like(w[k]) if accum0 is None else torch.tensor(np.asarray(accum0[k], np.float64))) for k in names}
    out = []
    for (x, pi, z) in batches:
        loss, _ = _tf_loss64(w, torch.tensor(x, dtype=torch.float64), torch.tensor(pi, dtype=torch.float64),
                             torch.tensor(z, dtype=torch.float64), blocks)
        grads = torch.autograd.grad(loss, [w[k] for k in names])
        gn = torch.sqrt(sum((g * g).sum() for g in grads))
        scale = clip / max(float(gn), clip)                                # tf.clip_by_global_norm
        with torch.no_grad():
            for k, g in zip(names, grads):
                g = g * scale
                accum[k] = momentum * accum[k] + g                         # MomentumOptimizer, use_nesterov=True:
                w[k] -= lr * g + lr * momentum * accum[k]                  #   var -= lr * grad + lr * momentum * accum
        out.append((float(loss.detach()), float(gn), {k: w[k].detach().numpy().copy() for k in names}))
    return out


@pytest.mark.parametrize("blocks,lr", [(1, 0.05), (2, 0.2)])
def test_train_step_matches_float64_restatement(blocks, lr):
    _check_train_step(blocks, lr, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("blocks,lr,upd_tol", [(2, 0.2, 2e-3), (7, 0.1, 5e-3)])
def test_train_step_on_device_matches_float64_restatement(blocks, lr, upd_tol):
    """The same check where the product trains: the module on cuda:0, forward AND backward through ROCm (MIOpen convolutions,
    fp32), 2 and 7 residual blocks, against the float64 restatement of the TF graph + MomentumOptimizer computed on the host,
    with MIOpen restricted to its deterministic kernels (Trainer(deterministic=True)): over 48 fresh processes on two boxes
    (round 3) every number of the 7-block case was bit-identical from run to run; loss within 2e-5, gradient norm within 2e-4,
    every tensor's two updates within 1.1e-3 of its largest update (kernels) — the tolerance is 2e-3 at 2 blocks, 5e-3 at 7."""
    _check_train_step(blocks, lr, "cuda:0", upd_tol, deterministic=True)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks,lr", [(2, 0.2), (7, 0.1)])
def test_train_step_on_device_fast_kernels(blocks, lr):
    """The kernels training really runs on (MIOpen's unrestricted choice: fp32 implicit GEMM, weight gradients reduced over
    split-K with atomics; 80x faster than the deterministic ones, train.deterministic_convolutions).  Their rounding differs
    from run to run and the 7-block case (15 batch-statistic BatchNorms, batch 12, clipped steps at lr 0.1) amplifies it: over
    110 fresh processes on five boxes (round 3; the last 30 in profiles/r03k_train_fast_probe.txt) the FIRST update stayed
    within 1.1e-3 on every kernel; the second within 4.3e-3 in 98 of them and, in the others, at 3e-2..1.3e-1 of the largest
    update on single output channels of mid-tower kernels (relative L2 error of those kernels' updates <= 1.5e-2, gradient norm
    off by up to 1.5e-4) — the same few discrete patterns on every box, i.e. which kernel MIOpen's search settled on.  So this
    test holds the first step to the bounds of the deterministic test (a wrong sign, slot, momentum or clip scale is an O(1)
    error there already) and, at 7 blocks, the second step to loss 1e-3, gradient norm 1e-2 and a relative L2 error of each
    kernel's update of 5e-2 (3x the worst of the 110 processes: the documented bound holds in EVERY process, no retry) — the
    second step is there to see momentum accumulate through the fast kernels.
    CZ_TRAIN_PROBE=1 prints the worst tensors of every step."""
    _check_train_step(blocks, lr, "cuda:0", 2e-3 if blocks == 2 else 6e-2, deterministic=False, first_step_only=blocks > 2)


def _check_train_step(blocks, lr, device, upd_tol=2e-3, deterministic=None, first_step_only=False):
    from cchess_zero_amd.net import PolicyValueModule
    from cchess_zero_amd.train import Trainer
    probe = os.environ.get("CZ_TRAIN_PROBE")
    m = PolicyValueModule(blocks, seed=4)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():   # non-zero biases: the L2 term covers them too
        for p in m.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    w0 = m.export_tf_layout()
    batches = [_batch(12, 3), _batch(12, 4)]
    ref = _run_restatement(w0, batches, lr, blocks)
    m = m.to(device)
    tr = Trainer(m, deterministic=deterministic)
    assert str(tr.device).startswith(device.split(":")[0])
    prev = w0
    for step, (x, pi, z) in enumerate(batches):
        acc, loss, gs = tr.train_step(x, pi, z, lr)
        rl, rgn, rw = ref[step]
        loose = first_step_only and step > 0
        if probe:
            print("PROBE", blocks, "det" if tr.deterministic else "fast", "step", step, "loss rel %.2e gradnorm rel %.2e"
                  % (abs(loss - rl) / abs(rl), abs(tr.last_grad_norm - rgn) / rgn), flush=True)
        assert gs == step + 1 and 0.0 <= acc <= 1.0
        assert abs(loss - rl) <= (1e-3 if loose else 2e-5) * abs(rl), (step, loss, rl)
        assert abs(tr.last_grad_norm - rgn) <= (1e-2 if loose else 2e-4) * rgn, (step, tr.last_grad_norm, rgn)
        now = m.export_tf_layout()
        worst, bad = [], []
        for k in rw:
            d_got = now[k].astype(np.float64) - prev[k].astype(np.float64)
            d_ref = rw[k] - (ref[step - 1][2][k] if step else np.asarray(w0[k], np.float64))
            scale = np.abs(d_ref).max()
            err = np.abs(d_got - d_ref).max()
            l2 = float(np.linalg.norm(d_got - d_ref) / np.linalg.norm(d_ref))
            worst.append((float(err / scale), l2, k))
            if loose:
                ok = l2 <= 5e-2 or d_ref.ndim == 1
            else:
                # conv biases in front of a batch-statistic BatchNorm have an analytically ZERO data gradient (the mean is
                # subtracted again): in fp32 what remains is cancellation noise, hence the small absolute term
                ok = err <= upd_tol * scale + 5e-6 * lr
            if not ok:
                bad.append((step, k, float(err), float(scale), l2))
        if probe:   # diagnostic: the three worst tensors of this step (max-abs and L2, relative)
            print("PROBE", blocks, "det" if tr.deterministic else "fast", "step", step,
                  [(round(e, 5), round(l2, 5), k) for e, l2, k in sorted(worst, reverse=True)[:3]], flush=True)
        assert not bad, bad
        prev = now
    # the moving statistics are never touched (quirk Q5: the reference never runs the update ops)
    for k, v in m.export_tf_layout().items():
        if k.startswith("bn"):
            assert np.array_equal(v, w0[k])


def test_clip_and_nan_check():
    from cchess_zero_amd.net import PolicyValueModule
    from cchess_zero_amd.train import Trainer
    m = PolicyValueModule(1, seed=0)
    tr = Trainer(m, global_norm=0.01)       # force clipping: the applied update has global norm 0.01 * lr
    w_before = torch.cat([p.detach().reshape(-1).clone() for p in m.parameters()])
    x, pi, z = _batch(6, 9)
    tr.train_step(x, pi, z, 1.0)
    w_after = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
    assert tr.last_grad_norm > 0.01
    # first Nesterov step from zero slots: delta = lr * (1 + momentum) * clipped gradient
    assert abs(float((w_after - w_before).norm()) - 0.01 * 1.9) < 1e-4
    bad = z.copy()
    bad[0, 0] = np.nan
    with pytest.raises(FloatingPointError):
        tr.train_step(x, pi, bad, 0.1)


def test_policy_update_control_flow_matches_reference_golden(golden_dir):
    """cchess_main.policy_update of the unmodified reference (main.py:1157-1204) was run through a stand-in self with a
    scripted net (tests/golden/gen_golden.py: gen_policy_update); the same scripted net through train.policy_update must
    take the same number of train steps at the same learning rates (early stop at kl > 4 * kl_targ), end with the same
    lr_multiplier (x / 1.5 adaptation, bounds 0.1 / 10), save the same step and log the same KL / explained variances."""
    import json
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from gen_golden import scripted_outputs   # imports nothing of the reference at module scope
    from cchess_zero_amd.train import policy_update
    g = np.load(os.path.join(golden_dir, "policy_update.npz"))
    states = [s.astype(np.float32) for s in g["states"]]
    buf = list(zip(states, list(g["pi"]), [float(z) for z in g["z"]]))
    cases = json.loads(str(g["meta"]))
    assert {c["steps"] for c in cases} == {1, 3, 5}
    for c in cases:
        class Net:
            k, lrs, saved, global_step = 0, [], None, 0

            def forward(self, sb):
                return scripted_outputs(sb, Net.k, c["scale"])

            def train_step(self, sb, pb, wb, lr):
                Net.k += 1
                Net.lrs.append(float(lr))
                Net.global_step = 100 + Net.k
                return 0.5, 1.25, Net.global_step

            def save(self, step):
                Net.saved = int(step)
        order = random.Random(99).sample(range(len(buf)), len(buf))   # the mini-batch order random.sample drew there (seed 99)
        lrm, info = policy_update(Net(), buf, len(buf), 5, 0.001, c["lrm"], 0.025, log=lambda *a: None, sample=order)
        assert Net.k == c["steps"] == info["steps"], c["name"]
        assert Net.lrs == c["lrs"], c["name"]
        assert lrm == c["lr_multiplier_after"], c["name"]
        assert Net.saved == c["saved_step"], c["name"]
        assert "{:.5f}".format(info["kl"]) == c["kl_logged"], (c["name"], info["kl"])
        assert "{:.3f}".format(info["explained_var_old"]) == c["explained_var_old_logged"], c["name"]
        assert "{:.3f}".format(info["explained_var_new"]) == c["explained_var_new_logged"], c["name"]


@pytest.mark.gpu
def test_policy_update_on_device(tmp_path):
    """policy_update with the real network on cuda:0 (fused fp16 forward, ROCm training step): the KL it reports is the
    reference's estimate recomputed here from forward() before / after the steps it took, the step count obeys the early
    stop, the weights moved and the checkpoint of the last step exists."""
    sys.path.insert(0, ROOT)
    from policy_value_network import policy_value_network
    from cchess_zero_amd.train import kl_estimate_rows, policy_update
    net = policy_value_network(2, save_dir=str(tmp_path), seed=3)
    x, pi, z = _batch(32, 6)
    buf = [(x[i], pi[i], float(z[i, 0])) for i in range(len(x))]
    old_l, _ = net.forward(list(x))
    w_before = torch.cat([p.detach().reshape(-1).clone() for p in net.module.parameters()])
    lrm, info = policy_update(net, buf, 32, 5, 0.02, 1.0, 0.025, log=lambda *a: None, sample=range(32))
    new_l, _ = net.forward(list(x))
    kl = float(np.mean(kl_estimate_rows(old_l, new_l)))
    assert 1 <= info["steps"] <= 5 and net.global_step == info["steps"]
    assert abs(kl - info["kl"]) <= 1e-6 * max(1.0, abs(kl)), (kl, info["kl"])
    assert info["steps"] == 5 or info["kl"] > 0.1
    assert lrm == (1.0 / 1.5 if info["kl"] > 0.05 else 1.5 if info["kl"] < 0.0125 else 1.0)
    w_after = torch.cat([p.detach().reshape(-1) for p in net.module.parameters()])
    assert float((w_after - w_before).abs().max()) > 0
    assert os.path.exists(os.path.join(str(tmp_path), "best_model.ckpt-%d.pt" % net.global_step))


class _CpuNet:
    """policy_value_network's training surface on a CPU module (the product class needs a HIP device)."""

    def __init__(self, blocks, save_dir):
        from cchess_zero_amd.net import PolicyValueModule
        from cchess_zero_amd.train import Trainer
        self.module = PolicyValueModule(blocks, seed=0)
        self.trainer = Trainer(self.module)
        self.save_dir = save_dir
        self.saved = []

    @property
    def global_step(self):
        return self.trainer.global_step

    def forward(self, positions):
        with torch.no_grad():
            lg, v = self.module(torch.as_tensor(np.asarray(positions, np.float32)).permute(0, 3, 1, 2))
        return lg.numpy(), v.numpy()

    def train_step(self, *a):
        return self.trainer.train_step(*a)

    def save(self, step):
        self.saved.append(int(step))


def _update_worker(rank, world, port, q, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from cchess_zero_amd.train import policy_update
    net = _CpuNet(1, tmp)
    x, pi, z = _batch(48, 21)          # every rank holds the same gathered buffer
    buf = [(x[i], pi[i], float(z[i, 0])) for i in range(len(x))]
    lrm, infos = 1.0, []
    # the second update uses a large learning rate: the KL estimate crosses 4 * kl_targ and the early stop must fire on
    # the same epoch everywhere
    for lr in (0.01, 0.5, 0.01):
        lrm, info = policy_update(net, buf, 16, 5, lr, lrm, 0.025, seed=5, log=lambda *a: None)
        infos.append((info["steps"], round(info["kl"], 12), lrm))
    flat = torch.cat([p.detach().reshape(-1) for p in net.module.parameters()])
    q.put((rank, infos, flat.numpy().tobytes(), net.saved, net.global_step))
    dist.monitored_barrier()   # gloo's host barrier: dist.barrier() first probes for a GPU, which opens the device in a CPU-only rank
    dist.destroy_process_group()


def test_policy_update_is_rank_consistent_gloo_world2(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_update_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (r0, i0, w0, s0, g0), (r1, i1, w1, s1, g1) = res
    assert i0 == i1, (i0, i1)                       # same number of steps, same all-reduced KL, same lr_multiplier
    assert w0 == w1                                 # replicas bit-identical after the updates
    assert g0 == g1 == sum(st for st, _, _ in i0)
    assert len(s0) == 3 and s1 == []                # only rank 0 writes checkpoints
    assert any(st < 5 for st, _, _ in i0), "the large-learning-rate update should stop early: %r" % (i0,)


@pytest.mark.gpu
def test_saver_keeps_the_five_most_recent_checkpoints(tmp_path, monkeypatch):
    """tf.train.Saver() default max_to_keep=5 (policy_value_network.py:148): one save per policy update must not fill the disk."""
    import glob
    import os
    import sys
    monkeypatch.chdir(tmp_path)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import policy_value_network as pv
    net = pv.policy_value_network(res_block_nums=1)
    for step in range(1, 9):
        net.save(step)
    left = sorted(glob.glob(os.path.join(net.save_dir, "best_model.ckpt-*.pt")))
    assert sorted(os.path.basename(f) for f in left) == sorted("best_model.ckpt-%d.pt" % i for i in range(4, 9))
    # a restart restores the newest one
    assert pv.policy_value_network(res_block_nums=1).global_step == 8
