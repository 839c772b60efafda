#!/usr/bin/env python3
"""Parameter sweep against separate calls, on one GPU (not part of bench.py's headline).

An 8-variant alpha_rot sweep (0.01 .. 100, values of se3icp.alpha_grid()) with the KITTI
driver's parameters over three workloads:

  bunny8   8 C2-like synthetic bunny problems (bench.py's C2 pairs, 41,670 points a cloud), se3_pt2pt
  shard8   an 8-pair KITTI-like shard (bench.py's C4 pairs 0..7, ~120k points a cloud), se3_gicp
  c4       the 64-pair C4 batch, se3_gicp (skipped when its largest group would not fit)

Per step, in this order and alternating so that drift hits all alike: the eight separate
se3icp_register_batch_device calls (the existing entry), then se3icp_register_sweep_device
at max_group 1, 2, 4, 8 and 0 (the engine's choice).  Every call ends synchronised, so a
host clock around it is the call's time.  One untimed warm-up step (buffers, code objects),
then --steps timed ones; medians with min / max.  The sweep's results are compared bitwise
with the separate calls' at these sizes before anything is timed.

Writes one JSON file (--out, default profiles/sweep_bench.json): per workload the times,
iterations per second, the separate calls' lrf_ms / setup_ms, the sweep's shared-setup and per-group setup times, the ratio
sweep / separate, and the time saved against (variants - 1) x the separate calls' setup.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "se3-icp_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

GROUPS = [1, 2, 4, 8, 0]


def sweep_alphas(se3icp):
    grid = se3icp.alpha_grid()
    want = [1 * 0.01, 5 * 0.01, 3 * 0.1, 1.0, 1.0 + 4 * 0.5, 10.0, 50.0, 100.0]
    assert all(a in grid for a in want)
    return want


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def same(a, b):
    return (np.array_equal(a.T, b.T) and a.num_iterations == b.num_iterations and a.status == b.status
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.scaling_factor == b.scaling_factor)


def run_workload(se3icp, torch, name, pairs, method, steps, warmup):
    variants = se3icp.sweep_params(se3icp.kitti_params(), alpha_rot=sweep_alphas(se3icp))
    nv, n = len(variants), len(pairs)
    d_src = torch.from_numpy(np.concatenate([s for s, _ in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([t for _, t in pairs])).cuda()
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    to = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
    torch.cuda.synchronize()
    points = int(so[-1] + to[-1])

    def separate():
        t0 = time.perf_counter()
        res, kts = [], []
        for v in variants:
            res.append(se3icp.register_batch_device(d_src.data_ptr(), so, d_tgt.data_ptr(), to, method, v))
            kts.append(se3icp.last_kernel_times())
        return time.perf_counter() - t0, res, kts

    def sweep(mg):
        t0 = time.perf_counter()
        res = se3icp.register_sweep_device(d_src.data_ptr(), so, d_tgt.data_ptr(), to, method, variants, max_group=mg)
        return time.perf_counter() - t0, res, se3icp.last_kernel_times()

    out = dict(workload=name, method=method, pairs=n, variants=nv, points=points, alphas=sweep_alphas(se3icp))
    # results first: bitwise, at the timed sizes
    _, want, _ = separate()
    differ = {}
    for mg in GROUPS:
        _, got, _ = sweep(mg)
        differ[str(mg)] = sum(not same(got[v][p], want[v][p]) for v in range(nv) for p in range(n))
    out["results_differing"] = differ
    iters = sum(r.num_iterations for row in want for r in row)
    out["iterations_total"] = iters
    for _ in range(max(0, warmup - 1)):
        separate()
        for mg in GROUPS:
            sweep(mg)
    t_sep, sep_lrf, sep_setup = [], [], []
    t_sw = {mg: [] for mg in GROUPS}
    sw_shared = {mg: [] for mg in GROUPS}
    sw_lrf = {mg: [] for mg in GROUPS}
    sw_group_setup = {mg: [] for mg in GROUPS}
    sw_loop = {mg: [] for mg in GROUPS}
    sw_groups = {}
    sep_loop = []
    for _ in range(steps):
        dt, res, kts = separate()
        t_sep.append(dt * 1e3)
        sep_lrf.append(sum(k["lrf_ms"] for k in kts))
        sep_setup.append(sum(k["setup_ms"] for k in kts))
        sep_loop.append(sum(row[0].time_loop_ms for row in res))
        for mg in GROUPS:
            dt, res, kt = sweep(mg)
            t_sw[mg].append(dt * 1e3)
            sw_shared[mg].append(kt["setup_ms"])
            sw_lrf[mg].append(kt["lrf_ms"])
            # one (setup, loop) time pair per group: every variant of a group reports its group's
            per_group = sorted({(row[0].time_setup_ms, row[0].time_loop_ms) for row in res})
            sw_groups[mg] = len(per_group)
            sw_group_setup[mg].append(sum(s - kt["setup_ms"] for s, _ in per_group))
            sw_loop[mg].append(sum(l for _, l in per_group))
    sep = statistics.median(t_sep)
    out["separate"] = dict(ms=med(t_sep), iterations_per_s=iters / (sep * 1e-3), lrf_ms_sum=med(sep_lrf),
                           setup_ms_sum=med(sep_setup), loop_ms_sum=med(sep_loop))
    shared_once = statistics.median(sep_setup) / nv  # a separate call's setup
    out["sweep"] = {}
    for mg in GROUPS:
        m = statistics.median(t_sw[mg])
        saved = sep - m
        ideal = (nv - 1) * shared_once
        out["sweep"][str(mg)] = dict(
            max_group=mg, groups=sw_groups[mg], ms=med(t_sw[mg]), iterations_per_s=iters / (m * 1e-3),
            ratio_to_separate=m / sep, shared_setup_ms=med(sw_shared[mg]), lrf_ms=med(sw_lrf[mg]),
            group_setup_ms_sum=med(sw_group_setup[mg]), loop_ms_sum=med(sw_loop[mg]), saved_ms=saved,
            ideal_saving_ms=ideal, shortfall_ms=ideal - saved,
            # where the rest went (GPU timeline): the groups' expansion + 12-D builds beyond what
            # the separate calls spend on 12-D builds is inside group_setup_ms_sum; a loop that got
            # slower or faster in lockstep is loop_ms_sum against the separate calls' loop_ms_sum
            loop_delta_ms=statistics.median(sw_loop[mg]) - statistics.median(sep_loop))
    print(json.dumps(dict(workload=name, separate_ms=sep,
                          sweep_ms={str(mg): statistics.median(t_sw[mg]) for mg in GROUPS}, differ=differ)), flush=True)
    del d_src, d_tgt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="bunny8,shard8,c4")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("sweep_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    import se3icp
    from bench import make_pairs
    se3icp.load()
    result = dict(tool="tools/sweep_bench.py", steps=args.steps, warmup=args.warmup,
                  device=torch.cuda.get_device_name(0), workloads=[])
    for wl in args.workloads.split(","):
        if wl == "bunny8":
            pairs, _ = make_pairs("C2", 8, 0, 8, 1975)
            result["workloads"].append(run_workload(se3icp, torch, wl, pairs, "se3_pt2pt", args.steps, args.warmup))
        elif wl == "shard8":
            pairs, _ = make_pairs("C4", 64, 0, 8, 1975)
            result["workloads"].append(run_workload(se3icp, torch, wl, pairs, "se3_gicp", args.steps, args.warmup))
        elif wl == "c4":
            pairs, _ = make_pairs("C4", 64, 0, 64, 1975)
            pts = sum(s.shape[0] + t.shape[0] for s, t in pairs)
            free, _ = torch.cuda.mem_get_info()
            if 8 * pts * 1024 > free:
                result["workloads"].append(dict(workload=wl, skipped=f"8 x {pts} points do not fit {free} free bytes"))
                continue
            result["workloads"].append(run_workload(se3icp, torch, wl, pairs, "se3_gicp", args.steps, args.warmup))
        else:
            sys.exit(f"unknown workload {wl}")
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
