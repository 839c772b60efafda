#!/usr/bin/env python3
"""One kd-tree order per cloud (se3icp_set_tree_sharing) against every slot building its own
trees, in one build on one GPU (not part of bench.py's headline; bench.py itself runs the
default mode).

For each of bench.py's workloads named (its pairs, method and parameters; C4 also as its first
8 pairs, "shard8"), one call at a time: se3icp_set_tree_sharing 1 (off, the parent's builds) and
0 (the default) alternate step by step, so that drift hits both alike.  Every call ends
synchronised, so a host clock around it is the call's time.  The results of the two modes are
compared bitwise before anything is timed.  --warmup untimed steps of each mode, then --steps
timed ones: median, min and max of the call and of the setup and loop phases,
se3icp_last_tree_stats of both modes and the loop's device-counted NN work (distance
evaluations and box tests: what a worse tree would cost).

C2's clouds are all distinct: nothing is adopted there, and its line is the path without a
donor against itself, to be held against mode 1's own min-max spread.  With SE3ICP_LIB naming a
library from before the switch (an A/B against the parent commit) only the default is timed.

Writes one JSON file (--out, default profiles/tree_adopt_bench.json).
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

WORK = ("se3_dist_evals", "se3_box_tests", "r3_dist_evals", "r3_box_tests")


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def same(a, b):
    return (a.T.tobytes() == b.T.tobytes() and a.num_iterations == b.num_iterations and a.status == b.status
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.scaling_factor == b.scaling_factor)


def run_workload(se3icp, torch, name, pairs, method, params, steps, warmup, has_switch):
    d_src = torch.from_numpy(np.concatenate([s for s, _ in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([t for _, t in pairs])).cuda()
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    to = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
    torch.cuda.synchronize()
    modes = (1, 0) if has_switch else (0,)

    def call(mode):
        if has_switch:
            se3icp.set_tree_sharing(mode)
        t0 = time.perf_counter()
        res = se3icp.register_batch_device(d_src.data_ptr(), so, d_tgt.data_ptr(), to, method, params)
        return time.perf_counter() - t0, res, se3icp.last_kernel_times()

    out = dict(workload=name, method=method, pairs=len(pairs), points=int(so[-1] + to[-1]))
    try:
        first = {}
        for m in modes:
            _, res, kt = call(m)
            first[m] = (res, kt)
            if has_switch:
                out.setdefault("tree_stats", {})["mode_1" if m else "default"] = se3icp.last_tree_stats()
        want = first[modes[0]][0]
        out["results_differing"] = sum(not same(a, b) for a, b in zip(first[0][0], want))
        out["iterations_total"] = sum(r.num_iterations for r in want)
        out["graph_stats"] = se3icp.last_graph_stats()
        out["loop_nn_work"] = {("mode_1" if m else "default"): {k: first[m][1][k] for k in WORK} for m in modes}
        if has_switch:
            out["loop_nn_work"]["ratio_default_to_mode_1"] = {
                k: (first[0][1][k] / first[1][1][k] if first[1][1][k] else 1.0) for k in WORK}
        for _ in range(warmup):
            for m in modes:
                call(m)
        keys = ("ms", "lrf_ms", "setup_ms", "loop_ms")
        acc = {m: {k: [] for k in keys} for m in modes}
        for _ in range(steps):
            for m in modes:
                dt, res, kt = call(m)
                a = acc[m]
                a["ms"].append(dt * 1e3)
                a["lrf_ms"].append(kt["lrf_ms"])
                a["setup_ms"].append(res[0].time_setup_ms)
                a["loop_ms"].append(res[0].time_loop_ms)
    finally:
        if has_switch:
            se3icp.set_tree_sharing(0)
    out["default"] = {k: med(v) for k, v in acc[0].items()}
    g = out["default"]["ms"]
    line = dict(workload=name, default_ms=g, differ=out["results_differing"])
    if has_switch:
        out["mode_1"] = {k: med(v) for k, v in acc[1].items()}
        b = out["mode_1"]["ms"]
        out["ratio"] = g["median"] / b["median"]
        out["saved_ms"] = b["median"] - g["median"]
        # a gain: the default's slowest step beats mode 1's fastest by more than mode 1's spread;
        # no loss: the default's median within mode 1's spread of mode 1's median
        out["gain_beyond_spread"] = b["min"] - g["max"] > b["max"] - b["min"]
        out["within_mode_1_spread"] = g["median"] <= b["median"] + (b["max"] - b["min"])
        line.update(mode_1_ms=b, setup_ms=[out["mode_1"]["setup_ms"], out["default"]["setup_ms"]],
                    loop_ms=[out["mode_1"]["loop_ms"], out["default"]["loop_ms"]], tree=out["tree_stats"]["default"])
    print(json.dumps(line), flush=True)
    del d_src, d_tgt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C4,shard8,C2,C3,C5")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_adopt_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tree_adopt_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    import bench
    import se3icp
    from se3icp import _lib, registration
    L = se3icp.load()
    registration.set_nn_events(False)  # as bench.py's timed steps
    has_switch = hasattr(L, "se3icp_set_tree_sharing")
    result = dict(tool="tools/tree_adopt_bench.py", steps=args.steps, warmup=args.warmup, has_switch=has_switch,
                  library=os.path.relpath(_lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0), workloads=[])
    made = {}
    for wl in args.workloads.split(","):
        base = "C4" if wl == "shard8" else wl
        if base not in bench.WORKLOADS:
            sys.exit(f"unknown workload {wl}")
        W = bench.WORKLOADS[base]
        if base not in made:
            made[base] = bench.make_pairs(base, W["batch"], 0, W["batch"], 1975)[0]
        pairs = made[base][:8] if wl == "shard8" else made[base]
        result["workloads"].append(run_workload(se3icp, torch, wl, pairs, W["method"],
                                                se3icp.default_params(**W["params"]), args.steps, args.warmup, has_switch))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
