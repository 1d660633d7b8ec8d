"""Parity of the EXACT product path bench.py times — SearchEngine.step with the fused net:
   cz_search_select (fp16 / bf16 x 16-channel planes) -> cz_net_trunk_f16 / _bf16 -> cz_fc_heads_f32 (value only)
   -> cz_search_expand_backup_fc (policy FC for the legal moves only)
at the BASELINE.json configurations (configs[1]: 4096 games x playout 400; configs[2]: 8192 games of a
playout-1600 search, crossing one cz_search_advance), against an oracle shadow on a subset of the trees.

The oracle (oracle/cchess_oracle.c, pinned to the unmodified reference) is fed, for its trees, the full logits row
of the policy FC restated in NumPy float32 (searchdrive.fc_logits_restated: the documented evaluation order of
k_expand_backup<FC>) from the z / value tensors READ BACK from the device between the net and the expansion
(step(tap=...)).  Everything the search does with the net's numbers — move generation, flip_policy, prior
normalisation, PUCT selection, backup, re-rooting — must then be bit-identical: root statistics and whole-tree
dumps are compared exactly.  (reference: MCTS_tree.main main.py:473-493, start_tree_search :350-435,
leaf_node.expand :175-187, update_tree :272-276, policy_value_network.forward policy_value_network.py:202-214)

A third test holds the bf16 fused net to the search-level effect that matters: bf16 vs the fp32 engine on the same
roots must pick the same most-visited root move for nearly all trees.
"""
import numpy as np
import pytest
import torch

import nethelpers
import searchdrive

pytestmark = pytest.mark.gpu


def _positions(G, seed):
    import bench
    from cchess_zero_amd.rules import Rules
    return bench.synth_positions(Rules(), G, seed)


class _Shadow:
    """Oracle search over trees `sub` of a HIP engine, fed the device's own z / value."""

    def __init__(self, eng, net, boards, side, rr, sub, cap):
        from oracle import oracle as O
        self.eng, self.net, self.sub = eng, net, np.asarray(sub)
        self.sub_t = torch.from_numpy(self.sub).to(eng.dev)
        self.orc = O.Search(len(self.sub), cap)
        self.orc.reset(boards.cpu().numpy()[self.sub], side.cpu().numpy()[self.sub], rr.cpu().numpy()[self.sub])
        self.w = net.pfc_w_rows.detach().cpu().numpy()
        self.b = net.pfc_b_f32.detach().cpu().numpy()
        self.steps = 0

    def tap(self, planes, z, value):
        self._z = z.index_select(0, self.sub_t).cpu().numpy()
        self._v = value.reshape(-1).index_select(0, self.sub_t).cpu().numpy()
        self._need = self.eng.need.index_select(0, self.sub_t).cpu().numpy()
        self._planes = planes.index_select(0, self.sub_t)[..., :14].float().cpu().numpy() if self.steps % 40 == 0 else None

    def step(self, mode):
        self.eng.step(self.net.forward_device, mode=mode, tap=self.tap)
        op, on = self.orc.select(mode)
        assert np.array_equal(on, self._need), "needs_eval differs at step %d" % self.steps
        if self._planes is not None:   # bf16 x 16 and f32 x 14 encodings of the same leaves
            assert np.array_equal(self._planes * on[:, None, None, None], op), "leaf planes differ at step %d" % self.steps
        self.orc.expand_backup(searchdrive.fc_logits_restated(self._z, self.w, self.b), self._v)
        self.steps += 1

    def compare(self, tag, dump_every=1):
        hs = self.eng.root_stats_host()
        os_ = self.orc.root_stats()
        for k in ("label", "N", "count"):
            assert np.array_equal(hs[k][self.sub], os_[k]), (tag, k)
        for k in ("Q", "P", "W"):
            assert np.array_equal(hs[k][self.sub].view(np.uint32), os_[k].view(np.uint32)), (tag, k)
        for i in range(0, len(self.sub), dump_every):
            assert np.array_equal(self.eng.tree_dump(int(self.sub[i]), 1 << 20), self.orc.tree_dump(i, 1 << 20)), (tag, i)
        return hs, os_


def _first_argmax_played(hs):
    """update_tree on the most visited root child, first maximum (what bench.py's advance_ply plays)."""
    N = hs["N"].astype(np.int64).copy()
    cnt = hs["count"].astype(np.int64)
    N[np.arange(N.shape[1])[None, :] >= cnt[:, None]] = -1
    best = N.argmax(axis=1)
    played = hs["label"][np.arange(len(best)), best].astype(np.uint16)
    played[cnt == 0] = 0xFFFF
    return played


def test_fused_step_configs1_4096x400_vs_oracle():
    """BASELINE.json configs[1]: 4096 games, playout 400, 7-block bf16 — the fused four-launch step for all 401
    steps; 64 trees shadowed by the oracle."""
    import bench
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.net import PolicyValueNet
    G, playouts = 4096, 400
    cap = bench.default_nodes_per_tree(playouts)
    boards, side, rr = _positions(G, 1000)   # bench.py's rank-0 seed
    net = PolicyValueNet(7, "cuda:0", torch.bfloat16, seed=0)
    assert net.fused_search
    eng = SearchEngine(G, cap, plane_dtype=torch.bfloat16, channels=16)
    eng.reset(boards, side, rr)
    sh = _Shadow(eng, net, boards, side, rr, np.arange(5, G, 64), cap)
    for step in range(playouts + 1):
        sh.step(0 if step == 0 else 1)
    hs, _ = sh.compare("configs[1]", dump_every=4)
    st, nodes, sims, depth = (x.cpu().numpy() for x in eng.status())
    assert not np.any(st) and np.all(sims == playouts)
    assert np.array_equal(hs["N"].sum(axis=1), np.full(G, playouts))
    print("configs[1] fused step: %d trees shadowed, mean leaf depth %.2f, mean nodes/tree %.0f" % (len(sh.sub), depth.mean(), nodes.mean()))


def test_fused_step_configs2_8192_playout1600_across_advance_vs_oracle():
    """BASELINE.json configs[2]: 8192 games of a playout-1600 search with the bench's node pools; 130 simulations,
    one cz_search_advance onto the most visited child (subtree kept), the root expansion of never-visited children
    and 100 more simulations; 32 trees shadowed by the oracle."""
    import bench
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.net import PolicyValueNet
    G, playouts = 8192, 1600
    cap = bench.default_nodes_per_tree(playouts)
    boards, side, rr = _positions(G, 1000)
    net = PolicyValueNet(7, "cuda:0", torch.float16, seed=0)      # bench.py's default engine
    eng = SearchEngine(G, cap, plane_dtype=torch.float16, channels=16)
    eng.reset(boards, side, rr)
    sh = _Shadow(eng, net, boards, side, rr, np.arange(3, G, 256), 40000)
    for step in range(131):
        sh.step(0 if step == 0 else 1)
    hs, os_ = sh.compare("before advance")
    played = _first_argmax_played(hs)
    assert np.array_equal(played[sh.sub], _first_argmax_played(os_))
    eng.advance(played)
    sh.orc.advance(played[sh.sub])
    hb, hsd, hrr = (x.cpu().numpy() for x in eng.root_state())
    ob, osd, orr = sh.orc.root_state()
    assert np.array_equal(hb[sh.sub], ob) and np.array_equal(hsd[sh.sub], osd) and np.array_equal(hrr[sh.sub], orr)
    for step in range(101):
        sh.step(0 if step == 0 else 1)
    hs, _ = sh.compare("after advance")
    st, nodes, sims, depth = (x.cpu().numpy() for x in eng.status())
    assert not np.any(st & ~8)
    assert np.all(sims[hs["count"] > 0] == 100)
    print("configs[2] fused step across an advance: %d trees shadowed, kept subtree + 100 sims: mean nodes/tree %.0f" % (len(sh.sub), nodes.mean()))


def test_fused_step_configs2_full_length_1600_playouts_vs_oracle():
    """BASELINE.json configs[2] at FULL length: 8192 games, the bench's node pools and default engine (7-block fp16), the
    root expansion + all 1600 simulations of a search (main.py:473-493), cz_search_advance onto the most visited child
    with the ~25 k-node subtree it keeps (update_tree, main.py:272-276), and 300 simulations of the next ply; 12 trees
    shadowed by the oracle for every one of the 1 902 lock-steps: needs-eval flags, root statistics and whole-tree
    dumps (60-75 k nodes per tree) bit-identical."""
    import bench
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.net import PolicyValueNet
    G, playouts = 8192, 1600
    cap = bench.default_nodes_per_tree(playouts)
    boards, side, rr = _positions(G, 1000)
    net = PolicyValueNet(7, "cuda:0", torch.float16, seed=0)
    eng = SearchEngine(G, cap, plane_dtype=torch.float16, channels=16)
    eng.reset(boards, side, rr)
    sh = _Shadow(eng, net, boards, side, rr, np.arange(11, G, 700), cap)
    for step in range(playouts + 1):
        sh.step(0 if step == 0 else 1)
    hs, os_ = sh.compare("1600 playouts")
    st, nodes, sims, depth = (x.cpu().numpy() for x in eng.status())
    assert not np.any(st & ~8) and np.all(sims == playouts)
    assert np.array_equal(hs["N"].sum(axis=1), np.full(G, playouts))
    n_full = nodes.copy()
    played = _first_argmax_played(hs)
    assert np.array_equal(played[sh.sub], _first_argmax_played(os_))
    eng.advance(played)
    sh.orc.advance(played[sh.sub])
    hb, hsd, hrr = (x.cpu().numpy() for x in eng.root_state())
    ob, osd, orr = sh.orc.root_state()
    assert np.array_equal(hb[sh.sub], ob) and np.array_equal(hsd[sh.sub], osd) and np.array_equal(hrr[sh.sub], orr)
    sh.compare("kept subtree")
    kept = eng.status()[1].cpu().numpy()
    for step in range(301):
        sh.step(0 if step == 0 else 1)
    hs, _ = sh.compare("next ply")
    st, nodes, sims, depth = (x.cpu().numpy() for x in eng.status())
    assert not np.any(st & ~8)
    print("configs[2] full length: %d trees shadowed over %d lock-steps; nodes/tree after 1600 playouts %.0f (max %d), kept by the "
          "advance %.0f, after 300 more %.0f; max leaf depth %d" % (len(sh.sub), sh.steps, n_full.mean(), n_full.max(), kept.mean(),
                                                                 nodes.mean(), depth.max()))


# (dtype, minimum root-argmax agreement, maximum mean visit L1).  Measured on an MI355X (1024 trees x 400 playouts):
# bf16 0.9453 / 0.0827, fp16 0.9854 / 0.0200; the CPU emulation of the two roundings (tests/agree_emulation.py, 48 trees)
# predicted 0.94 / 0.064 for bf16.  With a peaked, trained-like net PUCT amplifies the 0.9 % logit noise of a 15-layer
# bf16 tower (0.1 % for fp16) into a different most-visited move for a few trees in a hundred — a property of 16-bit
# inference, not of the kernels, whose arithmetic the two tests above pin exactly.  The thresholds sit just below the
# measured levels (10-15 trees of 1024: the fp32 side runs MIOpen's convolutions, whose choice of kernel — and with it the
# last bits of the fp32 logits — is not the same on every box): a numerically worse kernel fails.
# The STRICT engine (fp16 hi + lo halves, k_trunk_split_c128) is within 4e-5 of the fp32 logits on these weights: the
# searches must agree like two fp32 evaluations do — >= 0.999 of the most visited root moves, visit L1 <= 0.002.
# The MX engine (k_trunk_mx_c128: cross terms on a block-scaled fp6 MFMA, 30-40x closer to fp32 than "fp16"): the same bounds
# (measured 1.0000 / 0.0001, max |dP| 5.4e-7).
_AGREE = {"bf16": (torch.bfloat16, 0.93, 0.10, False), "fp16": (torch.float16, 0.975, 0.025, False),
          "strict": (torch.float16, 0.999, 0.002, True), "mx6": (torch.float16, 0.999, 0.002, "mx")}


@pytest.mark.parametrize("dname", ["bf16", "fp16", "strict", "mx6"])
def test_fused_search_agrees_with_fp32_engine(dname):
    """The fused 16-bit net (and the strict split engine) vs the fp32 engine (torch/MIOpen fp32 convs, full logits) on the same
    1024 roots, 400 playouts, trained-like weights: the root move a self-play game would most likely play (most visited child)
    and the visit distributions (L1 distance) are compared."""
    from cchess_zero_amd.engine import SearchEngine
    from cchess_zero_amd.net import PolicyValueModule, PolicyValueNet
    dtype, min_agree, max_l1, split = _AGREE[dname]
    G, playouts = 1024, 400
    boards, side, rr = _positions(G, 77)
    mod = PolicyValueModule(7, seed=3)
    a = PolicyValueNet(7, "cuda:0", dtype, module=mod, split=split)
    nethelpers.trained_like_(a)
    b = PolicyValueNet(7, "cuda:0", torch.float32, module=a.module, backend="torch")
    ea = SearchEngine(G, (playouts + 2) * 80, plane_dtype=dtype, channels=16)
    eb = SearchEngine(G, (playouts + 2) * 80, plane_dtype=torch.float32, channels=14)
    for e, n in ((ea, a), (eb, b)):
        e.reset(boards, side, rr)
        e.search(n.forward_device, playouts)
        assert not bool(e.status()[0].any())
    sa, sb = ea.root_stats_host(), eb.root_stats_host()
    assert np.array_equal(sa["label"], sb["label"])
    Na, Nb = sa["N"].astype(np.int64), sb["N"].astype(np.int64)
    agree = float((Na.argmax(axis=1) == Nb.argmax(axis=1)).mean())
    l1 = np.abs(Na - Nb).sum(axis=1) / float(playouts)       # L1 distance of the visit distributions, in [0, 2]
    top = np.sort(Nb, axis=1)[:, -1] / float(playouts)
    print("%s fused vs fp32 engine, %d trees x %d playouts: root argmax agreement %.4f, visit L1 mean %.4f max %.4f "
          "(mean top-move share %.3f, max |dP| %.3g)" % (dname, G, playouts, agree, l1.mean(), l1.max(), top.mean(),
                                                         np.abs(sa["P"] - sb["P"]).max()))
    assert agree >= min_agree
    assert l1.mean() <= max_l1


def test_schedule_optimisations_leave_full_batch_search_unchanged():
    """BASELINE configs[2] batch (8192 trees, 7-block fp16 fused net: bench.py's default), 200 simulations per tree, crossing one re-root:
    the product schedule bench.py times (simulations that need no net row completed inside the select launch, §4.8) and
    the opt-in evaluation cache (§4.9) against the plain one-simulation-per-step schedule — every root statistic of every
    tree (labels, N, W, Q, P bits) and every node count must be equal.  This is the size-independent form of the golden /
    oracle tree tests: whatever the number of trees, the REAL net returns the same bits for the same position, so
    completing a simulation early or lending an earlier evaluation cannot change a tree."""
    from cchess_zero_amd.engine import Context, SearchEngine
    from cchess_zero_amd.net import PolicyValueNet
    G, playouts, cap = 8192, 200, 200 * 96
    boards, side, rr = _positions(G, 1000)

    def run(extra, cache):
        ctx = Context(G, cap, 0)
        eng = SearchEngine(G, cap, 0, plane_dtype=torch.float16, channels=16, ctx=ctx)
        net = PolicyValueNet(7, "cuda:0", torch.float16, seed=0, ctx=ctx)
        if cache:
            eng.set_eval_cache(True)
        eng.reset(boards, side, rr)
        eng.set_terminal_extra(extra)
        out, steps = [], 0
        for ply in range(2):
            steps += eng.search(net.forward_device, playouts)
            rs = eng.root_stats()
            st, nodes, sims, _ = eng.status()
            assert bool(((sims == playouts) | ((st & ~8) != 0)).all().item())   # a tree that stopped (full pool, no moves) keeps its flag
            assert int(((st & ~8) != 0).sum().item()) < G // 100
            out.append({k: v.clone() for k, v in rs.items()})
            out[-1]["nodes"], out[-1]["status"], out[-1]["sims"] = nodes.clone(), st.clone(), sims.clone()
            n = rs["N"].clone()
            cnt = (rs["count"].to(torch.int64) & 0xFFFF).unsqueeze(1)
            n[torch.arange(128, device=n.device).unsqueeze(0) >= cnt] = -1
            played = rs["label"].gather(1, n.argmax(dim=1, keepdim=True)).squeeze(1)
            eng.advance(torch.where(cnt.squeeze(1) > 0, played, torch.full_like(played, -1)))
        hits = eng.eval_cache_stats() if cache else (0, 0)
        eng.set_terminal_extra(0)
        if cache:
            eng.set_eval_cache(False)
        return out, steps, hits

    ref, steps0, _ = run(0, False)
    assert steps0 == 2 * playouts
    for extra, cache in ((4, False), (4, True)):
        got, steps, hits = run(extra, cache)
        for ply in range(2):
            for k in ref[ply]:
                a, b = ref[ply][k], got[ply][k]
                if a.dtype.is_floating_point:
                    a, b = a.view(torch.int32), b.view(torch.int32)
                assert torch.equal(a, b), (extra, cache, ply, k)
        print("8192 trees x 2 plies x %d playouts, terminal_extra %d, cache %s: %d lock-steps instead of %d; cache hits %d / %d" %
              (playouts, extra, cache, steps, steps0, hits[0], hits[1]))
        assert steps <= steps0


def test_bench_times_k_steps_and_dumps_identical_outputs(tmp_path):
    """`bench.py --steps K --dump-outputs DIR`: the K steps are the only timed region and give ms_per_step; two runs with the
    same arguments dump the same arrays, bit for bit (float32, the search state and the last step's net outputs)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lines, dumps = [], []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--games", "512", "--playout", "64", "--steps", "24",
                            "--warmup", "4", "--age-steps", "48", "--no-cpu-baseline", "--dump-outputs", d],
                           capture_output=True, text=True, cwd=str(tmp_path), timeout=900, stdin=subprocess.DEVNULL)
        assert p.returncode == 0, p.stderr[-3000:]
        lines.append(json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1]))
        dumps.append({f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))})
    for line in lines:
        assert line["steps"] == 24 and line["contract_steps"]["steps"] == 24 and line["value_source"] == "contract_steps"
        assert line["steady_state"] is None and line["fast_engine"] is None and line["strict_engine"] is None
        assert line["ms_per_step"] == line["contract_steps"]["ms_per_step"] > 0
        # a plain run (no --full) measures nothing beyond its timed steps
        assert line["net_error"] is None and line["roofline_rules"] is None and line["cpu_baseline"] is None
        assert line["roofline"]["kernel"] == "k_trunk_mx_c128" and line["roofline"]["achieved"] > 0 and line["roofline"]["launches_timed"] >= 1
        assert "mfma_peak_measured_TFLOPs" not in line["roofline"]
    a, b = dumps
    assert {"root_N", "root_Q", "root_label", "tree_sims", "net_z", "net_value", "tree_index"} <= set(a) and set(a) == set(b)
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["root_N"].shape == (512, 128) and a["net_z"].shape == (512, 1, 90, 3) and a["root_N"].sum() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k
