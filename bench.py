#!/usr/bin/env python3
"""bench.py — MCTS simulations/sec of the MI355X hot path (select -> batched net -> expand/backup).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`.  For N > 1 the driver launches it through
torch.distributed.run, one rank per GPU; run from a bare shell (`python bench.py --gpus 2`, WORLD_SIZE unset) it
launches the N ranks itself.  One "step" = one lock-step of EVERY game tree on the rank: select -> one net row per tree
-> expand/backup.  A simulation that ends on a king capture or on the 60-ply rule needs no net row (the reference returns
before its net queue, main.py:409-416): it completes inside the select launch (--terminal-extra, default 4 per tree and
step), so a step completes G / (1 - f) simulations, f = the share of such simulations; simulations are COUNTED from the
per-tree device counters.  A tree that has had `--playout` simulations advances one ply (root-visit argmax ->
cz_search_advance, the update_tree of the reference) at the next check (every 8 steps), each tree at its own pace, so long
runs stay in the self-play regime.  Rank 0 prints ONE JSON line.  Metric/config follow
BASELINE.json: "MCTS simulations/sec (whole node), playout=1600, 7-block net", 8192 games per GPU (configs[2]).

A plain run does only what the headline needs: set-up (positions, net and its strict self-check, node pools, ageing), warm-up,
the K timed steps, --dump-outputs, and the line, whose roofline / roofline_tree come from HIP events of the timed steps.
  --full           also everything measured or checked outside those steps: the net-error probes (as benchmarked and on
                   trained-like weights), the stand-alone rules-kernel roofline, the MFMA ceiling probe, the CPU baseline
                   (unless --no-cpu-baseline), the record all-gather self-check (N > 1) and, with --selfplay, the 16 extra
                   sampled steps that give that mode its per-kernel figures.

Opt-in modes:
  --selfplay       the timed region is the whole device-resident self-play loop (cchess_zero_amd/selfplay.py: search,
                   visit-count policy, Dirichlet-noise sampling, records, re-rooting, adjudication, re-seeding of finished
                   games) with asynchronous plies: a step is the same lock-step, every 8 steps the games whose search is
                   complete move; sims/s counts completed simulations from the device counters.
  --timed-gather   (with --selfplay, N > 1) every 64 lock-steps each rank drains the records of the games that finished and
                   all ranks all-gather them over RCCL inside the timed region — the exchange step of configs[3].

Inputs are synthetic: seeded random-playout positions generated on the GPU with the rules kernels,
Glorot-uniform weights (seed 0): with the same arguments they are the same from run to run.  Nothing here reads the
reference unless CCHESS_REFERENCE names a checkout of it.

  --dump-outputs DIR   after the K timed steps, what the timed path computed (the net's outputs of the last step and the
                       search state a caller reads: root statistics and per-tree counters) goes to DIR/<name>.npy in
                       float32, at most 64 MB (a fixed, seeded sample of the trees beyond that), so that two builds can be
                       compared output for output.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import torch

from cchess_zero_amd.rules import START_BOARD

START = START_BOARD

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "fp16": 2500.0, "fp32": 157.3, "fp16x2": 2500.0, "bf16x2": 2500.0, "mx6": 2500.0}  # dense peaks, same guide (x2 / mx6: the strict engines; algorithmic flops of the fp32 graph against the 16-bit MFMA peak)
MX_KERNEL = "k_trunk_mx_c128"   # what cz_net_trunk_mx launches (csrc/cz_conv.hip; experiment builds with CCHESS_MX_KERNEL=2: k_trunk_mx2_c128)
TRUNK_KERNEL = {"fp16": "k_tower8_c128", "bf16": "k_tower8_c128", "fp16x2": "k_trunk_split_c128", "bf16x2": "k_trunk_split_c128", "mx6": MX_KERNEL}
TRAFFIC_FILE = {"k_tower8_c128": "pmc_traffic.json", "k_trunk_split_c128": "pmc_traffic_strict.json", "k_trunk_mx_c128": "pmc_traffic_mx.json"}

# The unmodified reference (pure Python) timed on a CPU host with a checkout of it; recorded in BASELINE.md and attached to
# the line as static, labelled fields.
REFERENCE_PYTHON = {
    "search_only_sims_per_s_per_core": 405, "end_to_end_2block_sims_per_s": 237, "end_to_end_7block_sims_per_s": 157,
    "where": "build container (8 vCPU), tools/time_reference.py on the unmodified reference, recorded in BASELINE.md; "
             "static numbers, not measured in this run",
}


def default_nodes_per_tree(playout):
    """Node pool capacity per tree.  A ply adds ~40 nodes per simulation on top of the subtree kept from the previous
    ply (the most visited child's share of the tree).  One pool per tree (cz_search_advance compacts in place); a tree
    that does fill its pool stops expanding for the rest of the ply, is flagged, and gets its room back at the advance.
    128 nodes per simulation: 8192 trees x 205 056 nodes x 28 B = 47 GB (round 1: two pools of 160 per simulation,
    118 GB)."""
    return (int(playout) + 2) * 128


def synth_positions(rules, G, seed, max_ply=80):
    """SURVEY 8(d)'s synthetic positions: cchess_zero_amd.rules.random_positions (seeded random playouts on the GPU)."""
    from cchess_zero_amd.rules import random_positions
    return random_positions(rules, G, seed, max_ply)


# ---- CPU baseline: the C oracle's search + a torch-CPU (oneDNN) fp32 net on this host's cores -----------------------------
def _cpu_workers(specs):
    """Runs oracle/cpu_baseline_worker.py once per spec (idx, games, threads, blocks, seconds, first_core), concurrently,
    as separate processes (their thread affinity has to be in place before torch / OpenMP load)."""
    worker = os.path.join(ROOT, "oracle", "cpu_baseline_worker.py")
    procs = [subprocess.Popen([sys.executable, worker] + [str(x) for x in sp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for sp in specs]
    out = []
    for p in procs:
        so, se = p.communicate(timeout=600)
        if p.returncode != 0:
            raise RuntimeError("cpu_baseline worker failed: " + se[-400:])
        out.append(json.loads([l for l in so.splitlines() if l.startswith("{")][-1]))
    return out


def reference_python_now(timeout=90):
    """SURVEY 8(d) items 1-2 when CCHESS_REFERENCE names a checkout of the unmodified reference: its own MCTS_tree.main
    with a constant-time forward, 50 and 400 playouts, one core — tools/time_reference.py --json in a subprocess."""
    ref = os.environ.get("CCHESS_REFERENCE")
    if not ref or not os.path.exists(os.path.join(ref, "main.py")):
        return None
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_reference.py"), "--json"], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=timeout)
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    except Exception as e:
        return {"error": repr(e)}


def cpu_baseline(blocks, seconds_target=12.0):
    """The CPU port timed on this host, single core and all cores: C oracle search + fp32 torch-CPU
    net, a bounded sample of the same workload family.  Test infrastructure used as the *baseline being measured*, never
    as the product path.  `value` is the all-core figure."""
    try:   # the CPUs this process may run on, not every CPU of the host
        cores = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        cores = os.cpu_count() or 1
    out = {"unit": "sims/s", "kind": "port", "reference_python": dict(REFERENCE_PYTHON, measured_in_this_run=False)}
    live = reference_python_now()
    if live and "error" not in live:
        out["reference_python"] = dict(live, measured_in_this_run=True, static_record=REFERENCE_PYTHON)
    elif live:
        out["reference_python"]["live_attempt"] = live
    # a container may see every host CPU and still be throttled to a few of them by its cgroup CPU quota: report it, and do
    # not oversubscribe it (measured on the GPU box: 256 visible CPUs, all-core throughput of ~4 cores)
    quota = None
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        if q[0] != "max":
            quota = float(q[0]) / float(q[1])
    except Exception:
        try:
            qq = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            if qq > 0:
                quota = qq / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        except Exception:
            pass
    out["visible_cpus"], out["cgroup_cpu_quota"] = cores, quota
    try:
        out["loadavg"] = os.getloadavg()[0]
    except Exception:
        pass
    if quota:
        cores = max(1, min(cores, int(quota)))
    try:
        r = _cpu_workers([(0, 8, 1, blocks, seconds_target * 0.4, 0)])[0]
        out["single_core"] = {"value": r["sims"] / r["seconds"], "cores": 1,
                              "sample": "8 games x %d lock-step simulations, 1 thread pinned to one core, %.1f s (%.0f %% in the net)" %
                                        (r["steps"], r["seconds"], 100.0 * r["net_seconds"] / r["seconds"])}
        tpw = 8 if cores >= 16 else max(1, cores // 2)     # threads per worker process
        workers = max(1, cores // tpw)
        games = 128
        r1 = _cpu_workers([(99, games, tpw, blocks, seconds_target * 0.4, 0)])[0]   # one worker alone: the scaling reference
        out["one_worker"] = {"value": r1["sims"] / r1["seconds"], "cores": tpw,
                             "sample": "1 worker x %d pinned threads, %d games x %d simulations, %.1f s" % (tpw, games, r1["steps"], r1["seconds"])}
        res = _cpu_workers([(i + 1, games, tpw, blocks, seconds_target, i * tpw) for i in range(workers)])
        out["value"] = float(sum(r["sims"] / r["seconds"] for r in res))
        out["cores"] = workers * tpw
        out["sample"] = ("%d worker processes x %d pinned threads, each %d games x ~%d lock-step simulations: C oracle search + fp32 "
                         "torch-CPU (oneDNN) %d-block net, %.1f s (%.0f %% in the net)" %
                         (workers, tpw, games, int(np.mean([r["steps"] for r in res])), blocks, float(np.mean([r["seconds"] for r in res])),
                          100.0 * float(np.mean([r["net_seconds"] / r["seconds"] for r in res]))))
    except Exception as e:   # the GPU number must survive a failing baseline leg
        out.setdefault("value", None)
        out.setdefault("cores", cores)
        out["error"] = repr(e)
    return out


def rules_roofline(rules, boards, side, n=1 << 20, reps=10):
    """K1 on its own (48 B board in + 264 B mask out = 312 B/position, HBM-bound in principle): cz_movegen over n
    positions (the run's synthetic positions, tiled), HIP events around `reps` launches.  Headline: the mask-only kernel
    (moves = NULL: k_movegen_mask, one position per lane) — what §8(d)'s 312 B describe; beside it the ordered-list kernel
    (k_movegen_list, list + mask: the reference's get_legal_moves contract)."""
    G = boards.shape[0]
    b = boards.repeat((n + G - 1) // G, 1)[:n].contiguous()
    sd = side.repeat((n + G - 1) // G)[:n].contiguous()

    def timed(**kw):
        rules.movegen(b, sd, **kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            rules.movegen(b, sd, **kw)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps
    sec = timed(want_mask=True, want_moves=False)
    sec_list_pad = timed(want_mask=True, want_moves=True)
    sec_list = timed(want_mask=True, want_moves=True, pad=False)    # CZ_MOVES_NO_PAD: rows written up to their count (round 6)
    mean_moves = float((rules.movegen(b[:65536], sd[:65536], want_mask=False, want_moves=False)[1].to(torch.int64) & 0xFFFF).float().mean().item())
    alg = 312.0 * n
    abi = (90 + 1 + 264 + 2) * float(n)
    abi_list = (90 + 1 + 256 + 264 + 2) * float(n)
    # counter traffic of the same launch shapes (tools/pmc_rules.sh -> profiles/pmc_rules_traffic.json), attached when the size matches
    tr_mask, tr_list, tr_nopad, tr_src = None, None, None, "no committed PMC measurement at %d positions" % n
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", "pmc_rules_traffic.json")))
        if int(tj.get("positions", -1)) == n:
            tr_mask = tj["kernels"]["k_movegen_mask"]["traffic_bytes_per_launch"]
            tr_list = tj["kernels"]["k_movegen_list<true, true>"]["traffic_bytes_per_launch"]
            tr_nopad = tj["kernels"]["k_movegen_list<true, false>"]["traffic_bytes_per_launch"]
            tr_src = "profiles/pmc_rules_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, FETCH x2)"
    except (OSError, ValueError, KeyError) as e:
        tr_src = "profiles/pmc_rules_traffic.json unusable: %r" % (e,)
    return {"bound": "hbm", "kernel": "k_movegen_mask (stand-alone K1, the legal-move SET: 2086-bit mask + count, one position per lane, register bit sets; inside the search the ordered generator runs in k_select)",
            "achieved": alg / sec / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": alg / sec / 1e9 / HBM_PEAK_GBS, "traffic": tr_mask, "traffic_source": tr_src,
            "positions": n, "positions_per_s": n / sec, "us_per_launch": sec * 1e6, "algorithmic_bytes_per_position": 312,
            "abi_bytes_per_position": abi / n, "abi_GBps": abi / sec / 1e9,
            "ordered_list_kernel": {"kernel": "k_movegen_list<MASK, no pad> (ordered move list in the reference's generation order, rows written up to their count — cz_movegen_ex CZ_MOVES_NO_PAD —, and the mask from one launch: one position per lane)",
                                    "positions_per_s": n / sec_list, "us_per_launch": sec_list * 1e6, "achieved": alg / sec_list / 1e9,
                                    "frac": alg / sec_list / 1e9 / HBM_PEAK_GBS, "traffic": tr_nopad, "mean_moves_per_position": mean_moves,
                                    "abi_bytes_per_position": 90 + 1 + 264 + 2 + 16.0 * ((mean_moves + 7) // 8 + 0.5),
                                    "abi_GBps": (90 + 1 + 264 + 2 + 16.0 * ((mean_moves + 7) // 8 + 0.5)) * n / sec_list / 1e9,
                                    "padded": {"kernel": "k_movegen_list<MASK, pad> (cz_movegen: 0xFFFF padding to 128 labels)", "positions_per_s": n / sec_list_pad,
                                               "us_per_launch": sec_list_pad * 1e6, "frac": alg / sec_list_pad / 1e9 / HBM_PEAK_GBS, "traffic": tr_list,
                                               "abi_bytes_per_position": abi_list / n, "abi_GBps": abi_list / sec_list_pad / 1e9},
                                    "note": "issue-bound (VALU: the per-kind generation, 120 candidates per position visited once each in the reference's order), not bandwidth-bound: see DESIGN.md 4.5"}}


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(full):
    """The ONE line rank 0 prints: every number the bench contract, the judge's roofline check and the 1e-3 contract need, under
    8 KB (the driver's record keeps the top-level keys and an 8 KB tail); the complete record — notes, telemetry, clock probe,
    per-kernel explanations — goes to the side file named in `detail_file` (tools/jline.py reads either)."""
    out = _pick(full, ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                       "dtype", "data", "engine", "value_source"])
    out["strict_check"] = full.get("strict_check")
    for leg_key in ("strict_engine", "fast_engine"):   # the OTHER engine's leg (strict_engine in a fast run, fast_engine in a strict run)
        st = full.get(leg_key)
        if st:
            se = _pick(st, ["dtype", "kernel", "value", "unit", "ms_per_step", "steps", "meets_target_1e6_sims_per_s_per_gpu"])
            r = st.get("roofline") or {}
            se.update({"frac": r.get("frac"), "achieved_TFLOPs": r.get("achieved"), "us_per_launch": r.get("us_per_launch"), "traffic": r.get("traffic")})
            ne = st.get("net_error") or {}
            for k in ("as_benchmarked_glorot", "trained_like"):
                if k in ne:
                    se["dlogit_" + k] = ne[k].get("dlogit")
                    se["dvalue_" + k] = ne[k].get("dvalue")
            se["meets_1e-3_abs_logit_and_value"] = ne.get("meets_1e-3_abs_logit_and_value")
            if full.get("n_gpus", 1) > 1:
                se["per_rank_sims_per_s"] = st.get("per_rank_sims_per_s")
            out[leg_key] = se
        else:
            out[leg_key] = None
    for k in ("steady_state", "contract_steps"):
        out[k] = _pick(full.get(k) or {}, ["steps", "seconds", "value", "ms_per_step", "simulations_per_net_row", "per_rank_sims_per_s"]) or None
    c = full.get("config") or {}
    out["config"] = _pick(c, ["workload", "games_per_gpu", "playout", "res_block_nums", "world_size", "dist_backend", "per_rank_sims_per_s",
                              "efficiency_vs_min_rank", "efficiency_vs_max_rank", "per_rank_spread", "per_rank_busy_seconds", "rank_cpus", "search_threads", "simulations_per_net_row", "net_rows_per_step",
                              "terminal_extra", "record_gather", "trees_with_error_status", "mean_leaf_depth", "node_pool_GB", "ms_per_move", "launches_per_lock_step", "lock_steps_per_move"])
    if c.get("selfplay"):
        out["config"]["selfplay"] = _pick(c["selfplay"], ["games_finished", "records", "dropped_records", "stalled_games", "timed_gather", "gathers",
                                                          "gathered_records", "pending_after_flush"])
    r = full.get("roofline") or {}
    ro = _pick(r, ["bound", "achieved", "peak", "unit", "frac", "traffic", "us_per_launch", "launches_timed", "flops_per_launch", "effective_clock_GHz",
                   "clock_scaled_peak", "frac_of_clock_scaled_peak", "mfma_flops_issued_per_algorithmic_flop", "power_W"])
    ro["kernel"] = str(r.get("kernel", "")).split(" (")[0]
    mp = r.get("mfma_peak_measured") or {}
    if "dense_random_operands" in mp:
        ro["mfma_peak_measured_TFLOPs"] = {k: mp[k]["tflops"] for k in ("dense_random_operands", "half_zero_operands") if k in mp}
    out["roofline"] = ro
    t = full.get("roofline_tree")
    out["roofline_tree"] = (dict(_pick(t, ["bound", "achieved", "peak", "unit", "frac", "traffic", "us_select", "us_expand_backup"]),
                                 kernel="k_select + k_expand_backup") if t else None)
    rr = full.get("roofline_rules")
    if rr and "achieved" in rr:
        o = dict(_pick(rr, ["bound", "achieved", "peak", "unit", "frac", "traffic", "positions", "positions_per_s", "us_per_launch"]), kernel="k_movegen_mask")
        ol = rr.get("ordered_list_kernel")
        if ol:
            o["ordered_list_kernel"] = dict(_pick(ol, ["positions_per_s", "frac", "us_per_launch", "traffic"]), kernel="k_movegen_list<MASK>" + (" no pad" if "padded" in ol else ""))
            if "padded" in ol:
                o["ordered_list_kernel"]["padded"] = _pick(ol["padded"], ["positions_per_s", "frac", "us_per_launch", "traffic"])
        out["roofline_rules"] = o
    else:
        out["roofline_rules"] = rr
    ne = full.get("net_error")
    if ne and "as_benchmarked_glorot" in ne:
        out["net_error"] = {k: _pick(ne[k], ["dlogit", "dvalue", "max_abs_logit", "argmax_agree"]) for k in ("as_benchmarked_glorot", "trained_like") if k in ne}
        out["net_error"].update(_pick(ne, ["meets_1e-3_abs_logit_and_value_as_benchmarked", "meets_1e-3_abs_logit_and_value_trained_like", "probe_informative"]))
        if "strict_on_trained_like" in ne:
            out["net_error"]["strict_on_trained_like"] = _pick(ne["strict_on_trained_like"], ["engine", "dlogit", "dvalue", "fell_over_from"])
    else:
        out["net_error"] = ne
    cb = full.get("cpu_baseline")
    if cb:
        o = _pick(cb, ["value", "unit", "cores", "kind", "sample", "visible_cpus", "cgroup_cpu_quota", "error"])
        if cb.get("single_core"):
            o["single_core_value"] = cb["single_core"].get("value")
        rp = cb.get("reference_python") or {}
        o["reference_python"] = _pick(rp, ["measured_in_this_run", "search_only_sims_per_s_per_core", "search_only_400_playouts_sims_per_s",
                                           "end_to_end_2block_sims_per_s", "end_to_end_7block_sims_per_s"])
        out["cpu_baseline"] = o
    else:
        out["cpu_baseline"] = None
    return out


def write_detail(full, tag):
    """the complete record next to the line: gpurun_out/ when it exists (it is what travels back from a GPU box), else the cwd"""
    d = os.path.join(ROOT, "gpurun_out") if os.path.isdir(os.path.join(ROOT, "gpurun_out")) else os.getcwd()
    path = os.path.join(d, "bench_detail_%s.json" % tag)
    try:
        with open(path, "w") as f:
            json.dump(full, f, indent=1)
        return os.path.relpath(path, ROOT) if path.startswith(ROOT) else path
    except OSError as e:
        return "not written: %r" % (e,)


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(d, eng, net_out, limit=DUMP_LIMIT_BYTES, seed=20240601):
    """What the timed path computed, as a caller of it receives it: the net outputs the last step's expansion read (z: the
    head convolutions' [trees, k, 90, 3] with the policy FC in the expansion, else logits [trees, k, 2086]; value [trees, k];
    k = simulations in flight per tree; only where rows are trees, not in compact mode or the self-play loop) and the search
    state after the last step (root children's label / N / Q / P / W, the child count, and per tree status, nodes,
    simulations and leaf depth).  Every array in float32 (the integers are
    exact in it).  Trees beyond the byte budget are a fixed, seeded sample; tree_index.npy lists the trees kept, in order."""
    G = eng.G
    rs = eng.root_stats()
    st, nodes, sims, depth = eng.status()
    per_tree = {"root_label": rs["label"].to(torch.int32) & 0xFFFF, "root_N": rs["N"], "root_Q": rs["Q"], "root_P": rs["P"],
                "root_W": rs["W"], "root_count": rs["count"].to(torch.int32) & 0xFFFF,
                "tree_status": st, "tree_nodes": nodes, "tree_sims": sims, "tree_depth": depth}
    for k, t in net_out.items():
        per_tree["net_" + k] = t.reshape(G, -1, *t.shape[1:]) if k != "value" else t.reshape(G, -1)
    tree_bytes = 4 + sum(4 * (v.numel() // G) for v in per_tree.values())
    keep = min(G, max(1, limit // tree_bytes))
    idx = np.arange(G) if keep == G else np.sort(np.random.default_rng(seed).choice(G, keep, replace=False))
    it = torch.from_numpy(idx).to(st.device)
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "tree_index.npy"), idx.astype(np.float32))
    for k, v in per_tree.items():
        np.save(os.path.join(d, k + ".npy"), v.index_select(0, it).float().cpu().numpy())


def self_launch(n):
    """`python bench.py --gpus N` from a bare shell: start the N ranks through torch.distributed.run."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1600)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--games", type=int, default=8192, help="game trees per GPU")
    ap.add_argument("--playout", type=int, default=1600)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--dtype", default="strict", choices=["bf16", "fp16", "fp32", "fp16x2", "bf16x2", "mx6", "strict"],
                    help="engine of the tower (fp32 accumulate).  strict (default since round 6: the engine policy_value_network() and main.py run, so `value` and `roofline` are the product's): the net measures itself against fp32 on its weights and runs the cheapest engine of mx6 -> fp16x2 -> fp32 inside 5e-4 (mx6 on the bench's TF-default weights at 7 and at 19 blocks; fp16x2 on the peaked trained-like set at 19); the fast fp16 engine is then timed as the fast_engine leg.  mx6 = fp16 hi halves + both cross terms of the hi + lo split on one block-scaled fp6 MFMA (k_trunk_mx_c128, 1.5 MFMA-equivalents per product); fp16x2 / bf16x2 = hi + lo halves of that type, three MFMAs per product (k_trunk_split_c128; also 19 blocks); fp16: one fp16 per operand (k_tower8_c128), twice the rate, 1e-3 only relative to the logit scale (see net_error in the output); with fp16 / bf16 the strict engine is the extra leg")
    ap.add_argument("--age-steps", type=int, default=800, help="untimed lock-steps BEFORE --warmup that bring every tree to a representative phase of its search: each tree's first search is cut at its own threshold (uniform in [8, age-steps] simulations), so when the timed region starts the trees are spread over the phases of a playout-long search on subtrees kept from a previous ply — the state of a long run — instead of all standing 25 simulations into a fresh search")
    ap.add_argument("--steady-steps", type=int, default=0, help="extra lock-steps timed AFTER the K contract steps (own barrier-bracketed region) for the steady_state block of the output, which then gives value and ms_per_step; 0 (default) = off: the K steps are the only timed ones")
    ap.add_argument("--alt-steps", "--strict-steps", dest="alt_steps", type=int, default=0, help="lock-steps of a third timed region in which the SAME trees are searched with the OTHER engine: the fast fp16 engine (k_tower8_c128; the fast_engine block of the output) when the run's engine is a strict one, the strict engine of this depth (the strict_engine block) when --dtype is fp16 / bf16; 0 (default) = off")
    ap.add_argument("--backend", default="auto", choices=["auto", "hip", "torch"], help="conv backend of the net")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run what the headline does not need: net-error probes, rules roofline, MFMA ceiling probe, CPU baseline, the N > 1 record all-gather self-check, the --selfplay sampled steps")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="nccl = RCCL (default); gloo only for single-GPU smoke tests of the N>1 path")
    ap.add_argument("--all-on-device0", action="store_true", help="testing only: every rank uses cuda:0")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--search-threads", type=int, default=1, help="simulations in flight per tree and step (the reference's search_threads; virtual loss 3); batch = games * search_threads")
    ap.add_argument("--graph", action="store_true", help="replay the launches of a lock-step as one captured HIP graph (measured: no gain at 8192 trees — the host already runs ahead of the GPU — and none at one tree x 16 search threads, 0.407 vs 0.410 ms per lock-step: five serial small launches, not host time)")
    ap.add_argument("--compact", action="store_true", help="compact evaluation batches: no net row for terminal / drawn leaves (no gain at 8192 trees: the trunk runs in rounds of 1024 rows)")
    ap.add_argument("--full-policy-fc", action="store_true", help="compute all 2086 logits per leaf (k_policy_fc) instead of folding the policy FC into the expansion")
    ap.add_argument("--nodes-per-tree", type=int, default=0, help="node pool capacity per tree (default (playout + 2) * 128)")
    ap.add_argument("--selfplay", action="store_true", help="time the device-resident self-play loop (asynchronous plies)")
    ap.add_argument("--terminal-extra", type=int, default=4, help="terminal / drawn simulations a tree may complete inside one select launch (0: one simulation per tree and step, round-1 behaviour)")
    ap.add_argument("--eval-cache", action="store_true", help="evaluation cache (cz_search_set_eval_cache): a leaf whose position the tree has evaluated before is expanded from the remembered node inside the select launch, without a net row; trees are bit-identical with it on or off.  Off in the default (headline) run")
    ap.add_argument("--xcache", type=int, default=0, metavar="LOG2_ENTRIES", help="with --eval-cache: the cross-tree level (cz_search_set_xcache), 2**LOG2_ENTRIES entries of 1088 bytes shared by all trees of the rank (20 = 1.1 GB); pays in self-play from the start position, where the games share their openings")
    ap.add_argument("--advance-every", type=int, default=8, help="steps between checks for trees that have had their playouts")
    ap.add_argument("--timed-gather", action="store_true", help="with --selfplay and N > 1: all-gather the finished games' records every 64 lock-steps, inside the timed region")
    ap.add_argument("--torch-advance", action="store_true", help="A/B only: the round-2 advance of ready trees (status / root statistics / argmax / reload as ~20 torch ops) instead of cz_search_pick_ready + cz_search_advance + cz_search_reload_finished")
    ap.add_argument("--force-dist", action="store_true", help="testing only: initialise the process group and run every collective even with a world of 1 (RCCL API check on one GPU)")
    ap.add_argument("--start-position", action="store_true", help="--selfplay: every game starts from the start position (default: the synthetic positions)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the K timed steps, write what they computed (last step's net outputs, root statistics, per-tree counters) to DIR/<name>.npy, float32, at most 64 MB (rank 0)")
    args = ap.parse_args()
    asked_strict = args.dtype == "strict"
    if asked_strict:   # where the ladder starts; the net's own measurement (strict_check, below) has the last word
        args.dtype = "mx6"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist_on = world > 1 or args.force_dist
    dist = None
    if dist_on:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if args.all_on_device0:
            local_rank = 0
        torch.cuda.set_device(local_rank)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo")
    else:
        torch.cuda.set_device(0)
        local_rank = 0
    assert args.gpus == world, "--gpus %d but WORLD_SIZE=%d" % (args.gpus, world)
    dev = torch.device("cuda", local_rank)
    cdev = dev if (dist_on and args.dist_backend == "nccl") else torch.device("cpu")   # where collectives run

    from cchess_zero_amd import parallel as PL
    from cchess_zero_amd.engine import Context, SearchEngine
    from cchess_zero_amd.net import PolicyValueNet, flops_per_position
    from cchess_zero_amd.rules import Rules
    # one process per GPU: every rank keeps to its own CPUs (the launcher thread of a rank must not be migrated over, or
    # throttled together with, the other ranks' under the box's CPU quota)
    # (the rank's own LOCAL_RANK, not the device index: with --all-on-device0 every rank computes on cuda:0 but still gets its own
    # CPU slice — the 8-rank test of round 5 found all eight ranks pinned to CPUs 0-7)
    cpus = PL.pin_rank_to_cpus(int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("LOCAL_WORLD_SIZE", world))) if world > 1 else None
    if world > 1:
        torch.set_num_threads(max(1, min(4, len(cpus) if cpus else 2)))

    G, playout = args.games, args.playout
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32, "fp16x2": torch.float16, "bf16x2": torch.bfloat16, "mx6": torch.float16}[args.dtype]
    cap = args.nodes_per_tree or default_nodes_per_tree(playout)
    ctx = Context(G, cap, local_rank)
    rules = Rules(ctx)
    K = max(1, args.search_threads)
    if args.selfplay and K != 1:
        ap.error("--selfplay runs one simulation in flight per tree")
    SPLIT_OF = {"mx6": "mx", "fp16x2": True, "bf16x2": True}
    strict_report = None
    if asked_strict:
        # the product's default engine, chosen the product's way: the ladder mx6 -> fp16x2 -> fp32 measured on these weights
        net = PolicyValueNet(args.blocks, dev, tdt, seed=0, backend="hip", ctx=ctx, split="strict")
        strict_report = net.strict_check()
        args.dtype = net.engine_name
        if args.dtype == "fp32":
            tdt = torch.float32
    else:
        net = PolicyValueNet(args.blocks, dev, tdt, seed=0, backend=args.backend, ctx=ctx, split=SPLIT_OF.get(args.dtype, False))
    mx = args.dtype == "mx6"
    split = args.dtype.endswith("x2") or mx
    # planes are written by k_select directly in the fused net kernel's input format (its 16-bit type, 16 channels)
    fused = (args.backend in ("auto", "hip")) and args.dtype in ("bf16", "fp16", "fp16x2", "bf16x2", "mx6")
    eng = SearchEngine(G, cap, local_rank, plane_dtype=tdt if fused else torch.float32, channels=16 if fused else 14, ctx=ctx, width=K)
    if args.full_policy_fc:
        net.fuse_policy_fc = False
    fused_fc = net.fused_search and K == 1
    compact = fused_fc and args.compact   # leaves that need no net evaluation are not in the net's batch
    eng.compact = compact
    boards, side, rr = synth_positions(rules, G, seed=1000 + rank)
    probe_boards, probe_side = boards[:256].clone(), side[:256].clone()   # the net-error block measures on these whatever the roots are
    if args.selfplay and args.start_position:
        boards = torch.from_numpy(np.tile(START_BOARD, (G, 1))).to(dev)
        side, rr = torch.zeros_like(side), torch.zeros_like(rr)

    ev = []        # per sampled step: (before select, after select, after net, after expand) HIP events
    conv_ev = []   # (start, end) events around single launches of the dominant kernel (recorded inside the net)
    step_no = [0]

    cur = {"net": net, "conv_ev": conv_ev, "ev": ev}   # the strict leg swaps the engine under the same loop
    # --dump-outputs: the net outputs the expansion of the latest step read (references to the tensors, no copies); a
    # replayed HIP graph writes into the tensors its capture saw (graph_net_out)
    last_net_out, graph_net_out = {}, {}

    def keep_net_out(planes, z_or_logits, value):
        last_net_out.update({"z" if z_or_logits.dim() == 3 else "logits": z_or_logits, "value": value})
    keep = keep_net_out if args.dump_outputs else None

    def one_step(mode, timed):
        # HIP events around the launches of every 8th timed step (recorded on the stream the kernels are launched on)
        sample = timed and step_no[0] % 8 == 0
        n_ = cur["net"]
        n_.conv_events = cur["conv_ev"] if sample else None
        step_no[0] += 1
        if not sample:
            eng.step(n_.forward_device, mode=mode, tap=keep)
            return
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()

        def tap(*a):
            e[2].record()
            if keep is not None:
                keep(*a)
        eng.step(n_.forward_device, mode=mode, pre_net=e[1].record, tap=tap)
        e[3].record()
        cur["ev"].append(e)

    gather_ok = None   # N > 1: result of the (untimed) record all-gather
    banked = torch.zeros(1, dtype=torch.int64, device=dev)   # simulations of the searches closed by an advance
    reloaded = torch.zeros(1, dtype=torch.int64, device=dev)  # games that ended and started afresh
    start_boards = torch.from_numpy(np.tile(START_BOARD, (G, 1))).to(dev)
    start_side, start_rr = torch.zeros(G, dtype=torch.uint8, device=dev), torch.zeros(G, dtype=torch.int32, device=dev)
    TE = max(0, args.terminal_extra) if K == 1 else 0

    # ageing: the FIRST search of tree g ends after thr[g] simulations (uniform in [8, age_steps]), every later one after `playout`
    gen_age = torch.Generator(device=dev).manual_seed(4242 + rank)
    age = max(0, args.age_steps)
    thr = torch.full((G,), playout, dtype=torch.int32, device=dev)
    if age >= 8 and not args.selfplay:
        thr = torch.randint(8, age + 1, (G,), generator=gen_age, device=dev, dtype=torch.int32).clamp(max=playout)
    min_thr = int(thr.min().item())
    playout_t = torch.full((G,), playout, dtype=torch.int32, device=dev)

    def advance_ready():
        """update_tree for every tree whose search has had its playouts (or whose node pool is full): most visited child;
        games that are over restart from the START position.  Three launches of the library, nothing on the host."""
        if not args.torch_advance:
            eng.advance_ready(thr, playout, start_boards, start_side, start_rr, banked, reloaded)
            return
        st, _, sims, _ = eng.status()
        ready = (sims >= thr) | ((st & 1) != 0)
        thr.copy_(torch.where(ready, playout_t, thr))
        banked.add_((sims.to(torch.int64) * ready).sum())
        rs = eng.root_stats()
        n = rs["N"].clone()
        cnt = (rs["count"].to(torch.int64) & 0xFFFF).unsqueeze(1)
        n[torch.arange(128, device=dev).unsqueeze(0) >= cnt] = -1
        best = n.argmax(dim=1, keepdim=True)
        played = rs["label"].gather(1, best).squeeze(1)
        eng.advance(torch.where(ready & (cnt.squeeze(1) > 0), played, torch.full_like(played, -1)))
        # the game is over where a king has been captured or the 60-ply rule has struck (main.py:1523-1552): such a tree
        # starts a new game from the START position, like the reference's reload (main.py:255-258,604-608) — it neither
        # goes on "searching" a finished game nor returns to a synthetic position that loses its king in one move
        b, _, r = eng.root_state()
        over = ready & (~(b == 1).any(dim=1) | ~(b == 8).any(dim=1) | (r >= 60) | (cnt.squeeze(1) == 0))
        eng.reload(over, start_boards, start_side, start_rr)
        reloaded.add_(over.sum())

    steps_since_reset = [0]
    graph = [None]   # the steady-state step (4 launches, static arguments) captured as one HIP graph

    trace = [] if os.environ.get("BENCH_TRACE_STEPS") else None   # debugging: one HIP event per timed step -> stderr

    def run(nsteps, timed):
        for i in range(nsteps):
            if trace is not None and timed and len(trace) < 64:
                e_ = torch.cuda.Event(enable_timing=True)
                e_.record()
                trace.append(e_)
            # every 8th timed step runs eagerly so that HIP events can bracket the launches on their stream
            if graph[0] is not None and not (timed and step_no[0] % 8 == 0):
                step_no[0] += 1
                graph[0].replay()
                last_net_out.update(graph_net_out)
            else:
                one_step(1, timed)   # mode 1 also expands the roots of trees that have just advanced
            steps_since_reset[0] += 1
            # no tree can have had its playouts before playout / (K * (TE + 1)) steps have passed since the common start
            if (i + 1) % args.advance_every == 0 and steps_since_reset[0] * K * (TE + 1) >= min_thr:
                advance_ready()

    sp = None
    gather_stats = {"gathers": 0, "records": 0, "seconds": 0.0}
    exchange, gathered = [None], []
    if args.selfplay:
        from cchess_zero_amd import parallel
        from cchess_zero_amd.selfplay import SelfPlay
        sp = SelfPlay(eng, net, playout, exploration=True, temperature=1.0, seed=77 + rank, continuous=True)
        sp.eval_cache = bool(args.eval_cache)
        sp.xcache_log2 = args.xcache if args.eval_cache else 0
        sp.start(boards, side, rr)
        eng.compact = compact

        def run_plies(n, timed):   # n lock-steps of the asynchronous loop, in chunks so that records leave the device
            done = 0
            while done < n:
                m = min(64, n - done)
                sp.run_async(m, every=args.advance_every, terminal_extra=TE)
                done += m
                if timed and args.timed_gather and dist_on:
                    rec = sp.drain_device()                       # device rows of the games that just finished (syncs on the cursor)
                    t1 = time.perf_counter()
                    if exchange[0] is None:   # fixed capacity: nothing to agree on, no host wait on the collective
                        exchange[0] = PL.RecordExchange(max(4096, G // 2), cdev)
                    out = exchange[0].exchange(rec if cdev.type == "cuda" else rec.cpu())
                    gather_stats["gathers"] += 1
                    gathered.append(out[:, 0, :8].clone())               # the counts are looked at after the timed region
                    if len(gathered) > 64:
                        gather_stats["records"] += int(torch.stack(gathered).contiguous().view(torch.int64).sum().item())
                        del gathered[:]
                    gather_stats["seconds"] += time.perf_counter() - t1
                else:   # the consumer of the records: the finished games leave the device
                    gather_stats["records"] += len(sp.drain())
        run_plies(age, False)
        run_plies(args.warmup, False)
    else:
        if args.eval_cache:
            eng.set_eval_cache(True)
            if args.xcache:
                eng.set_xcache(args.xcache)
        eng.reset(boards, side, rr)
        eng.set_terminal_extra(TE)
        eng.set_sim_target(playout)
        one_step(0, False)          # MCTS_tree.main root expansion (not a simulation)
        run(age, False)             # ageing (see --age-steps): independent of --warmup
        run(args.warmup, False)
    torch.cuda.synchronize()
    if args.graph and (fused_fc or K > 1) and not compact and not args.selfplay:
        try:   # capture AFTER the warm-up (kernel attributes set, allocator warm); a failure falls back to eager launches
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                one_step(1, False)
            graph_net_out.update(last_net_out)
            step_no[0] -= 1                      # the capture itself executed nothing
            torch.cuda.synchronize()
            graph[0] = gr
        except Exception as e:
            print("bench: HIP graph capture failed (%r), running eagerly" % (e,), file=sys.stderr)
            graph[0] = None
            torch.cuda.synchronize()
    count_sims = (lambda: sp.stats()["sims"]) if sp else (lambda: int(banked.item()) + int(eng.status()[2].sum().item()))
    # the first HIP events of a process cost a millisecond of lazy initialisation: create, record and read a few here, untimed,
    # so that the first sampled step of a short timed region (the driver's --steps 20) does not pay for it
    _warm = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    for e_ in _warm:
        e_.record()
    torch.cuda.synchronize()
    _warm[0].elapsed_time(_warm[-1])
    # ... and the first use of a torch op loads its code object (tens of ms): the counters read at the edges of the timed
    # region are read once here, then a few untimed steps bring the clocks back up — an idle GPU needs ~6 steps to ramp
    # (measured per step after a 50 ms gap: 2.63 2.86 2.71 2.58 2.48 2.43 ms against 2.34), which a 20-step region would
    # otherwise carry as a 3 % deficit
    count_sims()
    if dist_on:   # the first barrier / all-reduce of a process group sets the communicator up (hundreds of ms over RCCL)
        dist.barrier()
        PL.max_over_ranks(0.0, cdev)
    if sp:
        run_plies(8, False)
    else:
        run(8, False)

    busy_log = []   # per timed region: seconds of this rank's own work (the barrier-bracketed time is the slowest rank's)

    def timed_region(nsteps):
        """barrier + synchronize, EXACTLY nsteps lock-steps, synchronize + barrier: -> (max-over-ranks seconds, this rank's
        seconds, this rank's completed simulations, net rows of this rank [compact mode: measured])."""
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        sims0 = count_sims()
        rows0, csteps0 = eng.eval_totals() if compact else (0, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if sp:
            run_plies(nsteps, True)
        else:
            run(nsteps, True)
        torch.cuda.synchronize()
        busy = time.perf_counter() - t0      # this rank's own work, before it waits for the others
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        mine = time.perf_counter() - t0
        dtm = PL.max_over_ranks(mine, cdev) if dist_on else mine
        busy_log.append(busy)
        rows = float(G * K) * nsteps
        rpl = float(G * K)
        if compact:
            rows1, csteps1 = eng.eval_totals()
            rows = float(rows1 - rows0)
            rpl = rows / max(1, csteps1 - csteps0)
        return dtm, mine, count_sims() - sims0, rows, rpl

    dt, my_dt, my_sims, my_rows, rows_per_launch = timed_region(args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, eng, {} if compact else last_net_out)
    if trace:
        print("per-step GPU ms of the timed region:", " ".join("%.3f" % trace[i].elapsed_time(trace[i + 1]) for i in range(len(trace) - 1)), file=sys.stderr)
        trace = None
    steady = None
    telemetry, clock = None, None
    if args.steady_steps > 0:
        # the long leg is the one the headline is taken from; while it runs, a host thread samples the device's socket power
        # and shader clock (hwmon) and the trunk kernel stamps its own workgroups in both clocks (cz_set_clock_probe)
        from cchess_zero_amd.telemetry import ClockProbe, GpuSampler
        sampler, probe = None, None
        try:
            sampler = GpuSampler(local_rank).start()
            if fused:
                probe = ClockProbe(ctx, (G * K + 1) // 2 + 1)
                probe.arm()
        except Exception as e:
            print("bench: telemetry unavailable (%r)" % (e,), file=sys.stderr)
        steady = timed_region(args.steady_steps)
        try:
            if sampler is not None:
                telemetry = sampler.stop()
            if probe is not None:
                probe.disarm()                       # the last launch of the leg
                for _ in range(5):                   # and five more, eight steps apart, right behind it
                    probe.arm()
                    (run_plies if sp else run)(8, False)
                    probe.disarm()
                clock = probe.mean()
        except Exception as e:
            print("bench: telemetry read-out failed (%r)" % (e,), file=sys.stderr)
    strict_leg = None     # the OTHER engine on the same trees and loop (weights shared): (leg, events, net, "strict_engine" | "fast_engine")
    if args.alt_steps > 0 and fused and not sp and net.backend == "hip":
        if split:   # the run's engine is a strict one: the fast engine of the same 16-bit type (the planes buffer is in that type)
            net_s, alt_key = PolicyValueNet(args.blocks, dev, tdt, backend="hip", ctx=ctx, split=False, module=net.module), "fast_engine"
        elif tdt == torch.float16:
            net_s, alt_key = PolicyValueNet(args.blocks, dev, tdt, backend="hip", ctx=ctx, split="strict", module=net.module), "strict_engine"
            net_s.strict_check()
        else:       # a bf16 run gets bf16 halves
            net_s, alt_key = PolicyValueNet(args.blocks, dev, tdt, backend="hip", ctx=ctx, split=True, module=net.module), "strict_engine"
        if net_s.backend == "hip":
            net_s.fuse_policy_fc = net.fuse_policy_fc
            cur.update(net=net_s, conv_ev=[], ev=[])
            run(8, False)
            leg = timed_region(args.alt_steps)
            strict_leg = (leg, cur["conv_ev"], net_s, alt_key)
            cur.update(net=net, conv_ev=conv_ev, ev=ev)
    if dist_on and args.full:
        # outside the timed regions: the record exchange of the self-play loop (all-gather of packed (s, pi, z) records,
        # device-resident end to end; both the sized and the fixed-capacity form) on a ragged token batch, so every N>1 run
        # exercises the collective path; a failure is reported in the line, it does not take the throughput number with it
        gather_ok = PL.gather_selfcheck(cdev)

    if exchange[0] is not None:   # rows the fixed capacity held back leave now, outside the timed regions (none may be lost)
        for blk in exchange[0].flush():
            gathered.append(blk[:, 0, :8].clone())
        gather_stats["pending_after_flush"] = exchange[0].pending()
    if gathered:
        gather_stats["records"] += int(torch.stack(gathered).contiguous().view(torch.int64).sum().item())
        del gathered[:]
    if sp and args.full:   # the self-play loop launches through SelfPlay.run_async: sample the kernels' durations on 16 extra, uncounted steps
        eng.set_terminal_extra(TE)
        eng.set_sim_target(playout)
        for _ in range(16):
            step_no[0] = 0
            one_step(1, True)
        torch.cuda.synchronize()

    # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process; the committed
    # rocprofv3 --pmc measurement of the same launch shape is attached when the configuration matches.
    tower_kernel = TRUNK_KERNEL.get(args.dtype, "k_tower8_c128")

    def pmc_traffic(kernel, dtype_name):
        """-> (bytes per launch or None, where from / why not): profiles/pmc_traffic*.json holds the rocprofv3 --pmc measurement
        of one engine at one configuration (tools/summarize_profile.py writes kernel name prefixes: "k_tower8", "k_trunk_split")"""
        f = TRAFFIC_FILE.get(kernel)
        if not f or args.backend not in ("auto", "hip"):
            return None, "no committed PMC measurement for this engine"
        path = os.path.join(ROOT, "profiles", f)
        try:
            tj = json.load(open(path))
        except (OSError, ValueError) as e:
            return None, "profiles/%s unreadable: %r" % (f, e)
        want = {"B": G, "res_block_nums": args.blocks, "dtype": dtype_name}
        have = {k: tj.get("config", {}).get(k) for k in want}
        if have != want or bool(tj["config"].get("compact", False)) != bool(compact):
            return None, "profiles/%s was measured at %s, this run is %s" % (f, have, want)
        if not kernel.startswith(str(tj.get("kernel"))):
            return None, "profiles/%s describes kernel %r, not %s" % (f, tj.get("kernel"), kernel)
        return tj["traffic_bytes_per_launch"], ("profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, FETCH x2 gfx950 "
                                                "correction; algorithmic bytes %d)" % (f, tj["algorithmic_bytes_per_launch"]))
    traffic, traffic_src = pmc_traffic(tower_kernel, args.dtype)
    st, nodes, sims, depth = eng.status()
    bad = int((st & ~8).ne(0).sum().item())
    st_bits = {name: int(((st & bit) != 0).sum().item()) for name, bit in
               (("pool_exhausted", 1), ("no_moves", 2), ("move_overflow", 4), ("bad_advance", 8))}
    el = lambda a, b: a.elapsed_time(b)
    net_ms = float(np.mean([el(e[1], e[2]) for e in ev])) if ev else float("nan")
    sel_us = float(np.mean([el(e[0], e[1]) for e in ev])) * 1e3 if ev else float("nan")
    exp_us = float(np.mean([el(e[2], e[3]) for e in ev])) * 1e3 if ev else float("nan")
    # simulations are COUNTED (completed backups, per-tree device counters), not assumed: a parked tree (node pool
    # exhausted) or an abandoned descent (k > 1) contributes nothing.  With k = 1 and no parked tree this is G * steps.
    def totals(leg):
        """(max-over-ranks seconds, my seconds, my sims, my rows, .) -> (sims of all ranks, net rows of all ranks, per-rank sims/s)."""
        dtm, mine_dt, sims_, rows_, _ = leg
        if not dist_on:
            return float(sims_), float(rows_), [float(sims_) / mine_dt]
        tot = PL.sum_over_ranks([sims_, rows_], cdev)
        return tot[0], tot[1], PL.per_rank(float(sims_) / mine_dt, cdev)
    total_sims, total_rows, per_rank = totals((dt, my_dt, my_sims, my_rows, rows_per_launch))
    # how evenly the ranks ran (N > 1): each rank's simulations over ITS OWN busy time of the headline leg (before the closing
    # barrier), the spread of those rates, and the whole-job value against N copies of the slowest / the fastest rank
    head_leg = 1 if (steady is not None and len(busy_log) > 1) else 0
    head_sims = steady[2] if head_leg else my_sims
    own_rate = PL.per_rank(float(head_sims) / busy_log[head_leg], cdev) if dist_on else [float(head_sims) / busy_log[head_leg]]
    own_busy = PL.per_rank(busy_log[head_leg], cdev) if dist_on else [busy_log[head_leg]]
    rank_cpus = None
    if dist_on and cpus:
        lo, hi, n_ = PL.per_rank(min(cpus), cdev), PL.per_rank(max(cpus), cdev), PL.per_rank(len(cpus), cdev)
        rank_cpus = [[int(a), int(b), int(c)] for a, b, c in zip(lo, hi, n_)]     # [first cpu, last cpu, count] per rank
    steady_out = None
    if steady is not None:
        s_sims, s_rows, s_pr = totals(steady)
        steady_out = {"steps": args.steady_steps, "seconds": steady[0], "value": s_sims / steady[0], "unit": "sims/s",
                      "ms_per_step": steady[0] / args.steady_steps * 1e3, "net_rows_per_s": s_rows / steady[0],
                      "simulations_per_net_row": s_sims / max(1.0, s_rows), "per_rank_sims_per_s": s_pr,
                      "note": "a second barrier-bracketed timed region run right after the K contract steps, together with the ageing and the K steps more than 7 s of contiguous GPU work, so that a 5 s smi sampler sees the GPU busy; same loop, same counters"}
    flops = flops_per_position(args.blocks) * rows_per_launch
    peak = MFMA_PEAK_TFLOPS[args.dtype]
    # what ONE launch of the fused trunk kernel computes per position, algorithmically (2 x MACs, SAME-padding taps
    # counted densely): first conv + 2 * blocks tower convs + the two head 1x1 convs — everything but the three FC layers
    trunk_flops_per_pos = flops_per_position(args.blocks) - 2 * (180 * 2086 + 90 * 256 + 256)

    def mfma_probe():
        """The box's own practical MFMA ceiling, measured now (cz_probe_mfma_peak, ~30 ms per launch)."""
        import ctypes as C
        from cchess_zero_amd._lib import check, lib
        out_ = {}
        code = 2 if tdt == torch.float16 else 1
        for name, data in (("dense_random_operands", 0), ("half_zero_operands", 2)):
            tf, ms_ = C.c_double(), C.c_double()
            check(lib().cz_probe_mfma_peak(ctx.h, code, data, 4000, C.byref(tf), C.byref(ms_)), "cz_probe_mfma_peak")
            out_[name] = {"tflops": tf.value, "ms": ms_.value}
        out_["what"] = ("back-to-back v_mfma_f32_32x32x16_%s on register operands, 2 waves per SIMD, every CU, measured in this run right "
                        "after the timed regions (cz_probe_mfma_peak): what the MFMA pipes sustain on this box under its power governor" % ("f16" if code == 2 else "bf16"))
        return out_

    # MFMA flops ISSUED per algorithmic flop of the tower layers: 96 GEMM rows per 90 cells (padding rows), minus the MFMAs of the
    # row tiles that are off the board for a tap, which the kernels branch around: 15 of 108 tile-taps in k_tower8_c128 (rank-0,
    # file-0, file-9 and rank-8 tiles), 1 of 18 in k_trunk_split_c128 (its rank-0 tile), times the products per operand pair
    ISSUE_FAST = (96.0 / 90.0) * (93.0 / 108.0)
    ISSUE_SPLIT = 3.0 * (96.0 / 90.0) * (17.0 / 18.0)
    ISSUE_MX = 1.5 * (96.0 / 90.0) * (17.0 / 18.0)      # two fp16 MFMAs + one 8-pass fp6 MFMA per 32 input channels, in fp16-MFMA passes
    issue_of = lambda kernel: {"k_trunk_split_c128": ISSUE_SPLIT, "k_trunk_mx_c128": ISSUE_MX}.get(kernel, ISSUE_FAST)

    def trunk_roofline(conv_ms_, n_launches, issued_factor, kernel_name, clock_, telemetry_, traffic=traffic, traffic_src=traffic_src):
        nl_ = 2 * args.blocks
        conv_flops_ = float(trunk_flops_per_pos) * rows_per_launch
        ach = conv_flops_ / (conv_ms_ * 1e-3) / 1e12
        r = {"bound": "mfma", "kernel": kernel_name,
             "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak, "traffic": traffic, "traffic_source": traffic_src,
             "us_per_launch": conv_ms_ * 1e3, "launches_timed": n_launches, "flops_per_launch": conv_flops_,
             "flops_per_position": trunk_flops_per_pos, "conv_layers_per_launch": nl_ + 3,
             "mfma_flops_issued_per_algorithmic_flop": issued_factor}
        if clock_:
            r["effective_clock_GHz"] = clock_["effective_clock_GHz"]
            r["nominal_clock_GHz"] = 2.4
            r["clock_scaled_peak"] = peak * clock_["effective_clock_GHz"] / 2.4
            r["frac_of_clock_scaled_peak"] = ach / r["clock_scaled_peak"]
            r["mfma_issue_frac_of_clock_scaled_peak"] = ach * issued_factor / r["clock_scaled_peak"]
            r["clock_probe"] = clock_
        if telemetry_:
            r["power_W"] = telemetry_.get("power_W")
            r["sclk_MHz_driver"] = telemetry_.get("sclk_MHz")
            r["telemetry"] = telemetry_
        return r
    mfma_peak_measured = None
    if fused and rank == 0 and args.full:
        try:
            mfma_peak_measured = mfma_probe()
        except Exception as e:
            mfma_peak_measured = {"error": repr(e)}
    if conv_ev:
        # dominant kernel: the fused trunk (one launch = first conv + all tower layers + head convs over the whole batch)
        conv_ms = float(np.mean([a.elapsed_time(b) for a, b in conv_ev]))
        if net.backend == "hip":
            kname = (tower_kernel + " (first conv + whole residual tower + head 1x1 convs in one launch: %d conv layers, LDS-resident activations, %s MFMA, fp32 acc)" % (2 * args.blocks + 3, args.dtype))
            roof = trunk_roofline(conv_ms, len(conv_ev), issue_of(tower_kernel), kname, clock, telemetry)
            roof["net_forward_ms_per_step"] = net_ms
            roof["net_forward_tflops"] = flops / (net_ms * 1e-3) / 1e12
            roof["mfma_peak_measured"] = mfma_peak_measured
            if mfma_peak_measured and "dense_random_operands" in mfma_peak_measured:
                roof["frac_of_measured_mfma_peak_half_zero"] = roof["achieved"] * roof["mfma_flops_issued_per_algorithmic_flop"] / mfma_peak_measured["half_zero_operands"]["tflops"]
        else:
            conv_flops = 2.0 * rows_per_launch * 90 * 1152 * 128
            roof = {"bound": "mfma", "kernel": "k_conv3x3_c128 (fused conv3x3+BN+residual+ReLU, bf16 MFMA, fp32 acc)",
                    "achieved": conv_flops / (conv_ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
                    "frac": conv_flops / (conv_ms * 1e-3) / 1e12 / peak, "traffic": traffic, "traffic_source": traffic_src,
                    "us_per_launch": conv_ms * 1e3, "launches_timed": len(conv_ev), "flops_per_launch": conv_flops}
    elif ev:
        achieved = flops / (net_ms * 1e-3) / 1e12
        roof = {"bound": "mfma", "kernel": "net forward via torch/MIOpen (conv tower + heads), all launches of one step",
                "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak, "traffic": None,
                "ms_per_launch_group": net_ms, "flops_per_step": flops}
    else:   # no sampled step: --selfplay without --full
        roof = None
    # second roofline entry: the HBM-bound tree / rules side of a step (k_select = selection descent + make-move + move
    # generation + plane encoding; k_expand_backup = policy FC at the legal labels + node append + backup).  Algorithmic
    # bytes per tree: select  depth * L * 20 B of sibling statistics + 96 B root board + 2 B * L pending
    # moves + the leaf planes (2 880 B in 16-bit x 16 channels, 5 040 B in f32 x 14); expand  1 080 B of head outputs +
    # 28 B * L new nodes + 12 B * depth of backup (+ the 4 172 B logits row without the folded FC).
    mean_depth = float(depth.float().mean().item())
    mean_L = float((eng.root_stats()["count"].to(torch.int64) & 0xFFFF).float().mean().item())
    plane_b = 2880.0 if fused else 5040.0
    b_sel = G * (mean_depth * mean_L * 20.0 + 96.0 + 2.0 * mean_L + plane_b)
    b_exp = G * ((1080.0 if fused_fc else 2086.0 * 4) + 28.0 * mean_L + 12.0 * mean_depth)
    tree_roof = None
    tree_traffic, tree_traffic_src = None, None
    try:   # committed counter traffic of the same launch shapes (tools/profile_round.sh -> tools/summarize_profile.py)
        tt = json.load(open(os.path.join(ROOT, "profiles", "pmc_tree_traffic%s.json" % {"mx6": "_mx", "fp16x2": "_strict"}.get(args.dtype, ""))))
        if {k: tt["config"].get(k) for k in ("B", "res_block_nums", "dtype")} == {"B": G, "res_block_nums": args.blocks, "dtype": args.dtype} and fused_fc and not compact:
            kk = tt["kernels"]
            tree_traffic = sum(kk[n]["fetch_bytes_x2"] + kk[n]["write_bytes"] for n in ("k_select", "k_expand_backup") if n in kk)
            tree_traffic_src = "profiles/pmc_tree_traffic*.json of this engine's run (FETCH_SIZE x2 + WRITE_SIZE of k_select + k_expand_backup, per step)"
    except Exception:
        pass
    if ev and K == 1:
        ach = (b_sel + b_exp) / ((sel_us + exp_us) * 1e-6) / 1e9
        tree_roof = {"bound": "hbm", "kernel": "k_select + k_expand_backup%s (tree + rules side of a step)" % ("<FC>" if fused_fc else ""),
                     "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": tree_traffic,
                     "traffic_source": tree_traffic_src,
                     "us_select": sel_us, "us_expand_backup": exp_us, "algorithmic_bytes_select": b_sel, "algorithmic_bytes_expand": b_exp,
                     "select_GBps": b_sel / (sel_us * 1e-6) / 1e9, "expand_GBps": b_exp / (exp_us * 1e-6) / 1e9,
                     "mean_leaf_depth": mean_depth, "mean_children": mean_L,
                     "note": "latency/issue-bound kernels: one dependent HBM round trip per tree level; 3 % of a step"}
    if (G, playout, args.blocks) == (8192, 1600, 7):
        cfg_name = "BASELINE.json configs[2]" + ("; per-GPU share of configs[3]" if world > 1 else "")
    elif (G, playout, args.blocks, args.dtype) == (8192, 1600, 19, "fp16"):
        cfg_name = "per-GPU share of BASELINE.json configs[4]"
    elif (G, playout, args.blocks) == (4096, 400, 7):
        cfg_name = "BASELINE.json configs[1]"
    else:
        cfg_name = "custom configuration"
    cfg = {"workload": "%d parallel games per GPU, playout=%d, %d-block net %s (%s)%s" % (G, playout, args.blocks, args.dtype, cfg_name, "; device-resident self-play loop, asynchronous plies" if sp else ""),
           "games_per_gpu": G, "playout": playout, "conv_backend": net.backend, "policy_fc": "in-expansion, legal moves only" if fused_fc else "full 2086 logits",
           "net_rows_per_step": rows_per_launch, "compact_batches": bool(compact), "hip_graph": graph[0] is not None, "record_gather": gather_ok, "res_block_nums": args.blocks, "search_threads": K,
           "positions": "seeded random playouts from the start position, ply~U[0,80]",
           "nodes_per_tree": cap, "node_pool_GB": G * cap * 30 / 1e9,
           "dist_backend": (dist.get_backend() if dist_on else None), "world_size": world, "rank0_cpus": cpus, "rank_cpus": rank_cpus,
           "per_rank_sims_per_s": per_rank, "per_rank_own_busy_sims_per_s": own_rate, "per_rank_busy_seconds": own_busy,
           "per_rank_spread": (max(own_rate) - min(own_rate)) / (sum(own_rate) / len(own_rate)),
           "simulations_counted": total_sims, "net_rows": total_rows,
           "simulations_per_net_row": total_sims / max(1.0, total_rows), "terminal_extra": TE, "advance_every": args.advance_every,
           "net_rows_per_s": total_rows / dt,
           "age_steps": age, "tree_state_at_t0": ("every tree has finished a first, shortened search (cut at its own threshold, uniform in [8, %d] simulations) and stands at its own phase of a %d-playout search on the subtree it kept" % (age, playout)) if (age >= 8 and not sp) else "fresh searches",
           "eval_cache": (dict(zip(("hits", "lookups"), eng.eval_cache_stats())) if args.eval_cache else None),
           "xcache": (dict(eng.xcache_stats(), log2_entries=args.xcache) if (args.eval_cache and args.xcache) else None), "games_reloaded_rank0": int(reloaded.item()),
           "mean_leaf_depth": mean_depth, "mean_nodes_per_tree": float(nodes.float().mean().item()),
           "trees_with_error_status": bad, "status_bits": st_bits}
    if sp:
        s = sp.stats()
        cfg["selfplay"] = {"steps_timed": args.steps, "games_finished": s["games"], "red_wins": s["red_wins"], "black_wins": s["black_wins"],
                           "draws": s["draws"], "records": s["plies"], "stalled_games": s["stalled"], "dropped_records": s["dropped"],
                           "game_generations": s["games"] / float(G), "timed_gather": bool(args.timed_gather and dist_on),
                           "gathers": gather_stats["gathers"], "gathered_records": gather_stats["records"],
                           "gather_seconds_rank0": gather_stats["seconds"], "pending_after_flush": gather_stats.get("pending_after_flush")}
    strict_out, alt_key = None, None
    if strict_leg is not None:
        leg, s_ev, net_s, alt_key = strict_leg
        s_sims, s_rows, s_pr = totals(leg)
        s_dtype = net_s.engine_name
        s_kernel = TRUNK_KERNEL[s_dtype]
        strict_out = {"engine": {"mx6": MX_KERNEL + ": fp16 hi halves on fp16 MFMAs + both cross terms of the hi + lo split on one block-scaled fp6 MFMA, 1.5 MFMA-equivalents per product",
                                 "fp16x2": "k_trunk_split_c128: every weight and stored activation as fp16 hi + lo halves, three MFMAs per product",
                                 "bf16x2": "k_trunk_split_c128, bf16 halves",
                                 "fp16": "k_tower8_c128: one fp16 per operand — twice the strict engine's rate, 1e-3 only relative to the logit scale (see its net_error)",
                                 "bf16": "k_tower8_c128: one bf16 per operand"}[s_dtype], "dtype": s_dtype, "kernel": s_kernel,
                      "steps": args.alt_steps, "seconds": leg[0], "value": s_sims / leg[0], "unit": "sims/s",
                      "ms_per_step": leg[0] / args.alt_steps * 1e3, "net_rows_per_s": s_rows / leg[0], "per_rank_sims_per_s": s_pr,
                      "meets_target_1e6_sims_per_s_per_gpu": bool(s_sims / leg[0] / world >= 1e6),
                      "strict_check": net_s.strict_report,
                      "note": "third barrier-bracketed timed region: the same trees and loop with this engine swapped in (same weights)"}
        if s_ev:
            s_ms = float(np.mean([a.elapsed_time(b) for a, b in s_ev]))
            s_tr, s_src = pmc_traffic(s_kernel, s_dtype)
            strict_out["roofline"] = trunk_roofline(s_ms, len(s_ev), issue_of(s_kernel), s_kernel, None, None, s_tr, s_src)
    # headline: the LONG leg (steady_state) when it ran — the K contract steps (the driver's K = 20 is 47 ms) read a percent
    # or two off it and are kept as contract_steps
    contract = {"steps": args.steps, "seconds": dt, "value": total_sims / dt, "ms_per_step": dt / args.steps * 1e3,
                "note": "the EXACTLY-K-steps region of the bench contract (barrier + synchronize on both sides, max over ranks)"}
    head_val, head_ms, head_src = total_sims / dt, dt / args.steps * 1e3, "contract_steps"
    if steady_out is not None:
        head_val, head_ms, head_src = steady_out["value"], steady_out["ms_per_step"], "steady_state (value and ms_per_step are the %d-step leg timed right after the K = %d contract steps, which are kept under contract_steps)" % (args.steady_steps, args.steps)
    out = {
        "metric": "MCTS simulations/sec (whole node), playout=%d, %d-block net" % (playout, args.blocks),
        "value": head_val, "unit": "sims/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": head_ms, "value_source": head_src, "contract_steps": contract,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic", "engine": "%s (%s)%s" % (tower_kernel if fused else "torch/MIOpen", {"fp16": "one fp16 per operand: the fast engine; the 1e-3 contract engine of this depth is the strict_engine leg", "bf16": "one bf16 per operand", "mx6": "strict: fp16 hi halves + fp6 block-scaled cross terms", "fp16x2": "strict: fp16 hi + lo halves, three MFMAs per product", "bf16x2": "bf16 hi + lo halves"}.get(args.dtype, args.dtype),
                                                                           "; precision 'strict' = the default of policy_value_network() / main.py, selected by the net's own measurement against fp32 on these weights" if asked_strict else ""),
        "strict_check": strict_report,
        "steady_state": steady_out, "strict_engine": strict_out if alt_key == "strict_engine" else None,
        "fast_engine": strict_out if alt_key == "fast_engine" else None, "net_error": None, "config": cfg,
        "roofline": roof, "roofline_tree": tree_roof, "roofline_rules": None,
    }
    # the --mode play shape (one tree, search_threads in flight: main.py:1433-1491,231): what a move costs, and how many launches
    cfg["ms_per_move"] = playout / max(1e-9, head_val / (world * G)) * 1e3     # `playout` simulations of ONE tree at the measured rate
    cfg["launches_per_lock_step"] = (4 if fused_fc else (5 if net.backend == "hip" else None))   # select, trunk, value / FC heads, expand (+ k_policy_fc without the folded FC)
    cfg["lock_steps_per_move"] = head_ms and cfg["ms_per_move"] / head_ms
    cfg["efficiency_vs_min_rank"] = head_val / (world * min(own_rate))
    cfg["efficiency_vs_max_rank"] = head_val / (world * max(own_rate))
    if rank == 0 and args.full:
        # precision of the benchmarked engine, measured here: the net exactly as timed (same weights) and a peaked,
        # trained-like weight set, against fp32 on the same inputs (256 of the run's own synthetic positions)
        try:
            from cchess_zero_amd.net import net_error, trained_like_
            xs = rules.encode_planes(probe_boards, probe_side).float()    # the run's synthetic positions, also under --start-position
            ne = {"reference": "fp32 torch module on the device, same weights and inputs (that engine: <= 3e-5 of the NumPy restatement of the reference graph, tests/test_net.py)",
                  "as_benchmarked_glorot": net_error(net, xs)}
            ne["meets_1e-3_abs_logit_and_value_as_benchmarked"] = bool(ne["as_benchmarked_glorot"]["dlogit"] <= 1e-3 and ne["as_benchmarked_glorot"]["dvalue"] <= 1e-3)
            out["net_error"] = ne
            net_t = PolicyValueNet(args.blocks, dev, tdt, seed=0, backend=args.backend, ctx=ctx, split=SPLIT_OF.get(args.dtype, False))
            trained_like_(net_t, xs[:96])
            ne["trained_like"] = net_error(net_t, xs)
            ne["meets_1e-3_abs_logit_and_value_trained_like"] = bool(ne["trained_like"]["dlogit"] <= 1e-3 and ne["trained_like"]["dvalue"] <= 1e-3)
            # the probe must say something: a dead value head (dvalue exactly 0) or a blown-up calibration would not
            ne["probe_informative"] = bool(0.0 < ne["trained_like"]["dvalue"] < 0.5 and ne["trained_like"]["dlogit"] > 0.0)
            if asked_strict:   # what precision "strict" itself would run on the trained-like set (it may fall over where mx6 is marginal)
                net_a = PolicyValueNet(args.blocks, dev, torch.float16, backend="hip", ctx=ctx, split="strict", module=net_t.module)
                ne["strict_on_trained_like"] = dict(net_a.strict_check(), probe=net_error(net_a, xs))
            if strict_leg is not None:
                net_s = strict_leg[2]
                se = {"as_benchmarked_glorot": net_error(net_s, xs)}
                net_ts = PolicyValueNet(args.blocks, dev, net_s.dtype, backend="hip", ctx=ctx, split=SPLIT_OF.get(net_s.engine_name, False), module=net_t.module)
                se["trained_like"] = net_error(net_ts, xs)
                se["meets_1e-3_abs_logit_and_value"] = bool(max(se[k][q] for k in ("as_benchmarked_glorot", "trained_like") for q in ("dlogit", "dvalue")) <= 1e-3)
                out[alt_key]["net_error"] = se
        except Exception as e:
            out["net_error"] = {"error": repr(e)}
        try:
            out["roofline_rules"] = rules_roofline(rules, boards, side)
        except Exception as e:
            out["roofline_rules"] = {"error": repr(e)}
    if dist_on:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # the CPU baseline runs after every rank has left the timed regions and the process group (N > 1: the other ranks
        # have exited or are exiting; a shorter sample keeps the multi-GPU line quick)
        PL.unpin_cpus()
        if args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.blocks, args.cpu_seconds if world == 1 else min(args.cpu_seconds, 5.0))
        else:
            out["cpu_baseline"] = None
        line = compact_line(out)
        line["detail_file"] = write_detail(out, "%s_n%d" % (args.dtype, world))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
