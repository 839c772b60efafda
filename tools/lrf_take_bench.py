#!/usr/bin/env python3
"""Taking a cloud's first class's neighbour lists in its later classes (se3icp_set_lrf_taking)
against the seeded selection, in one build on one GPU (not part of bench.py's headline; bench.py
itself runs the default mode).

For each of bench.py's workloads named (its pairs, method and parameters; C4 also as its first
8 pairs, "shard8"), one call at a time: se3icp_set_lrf_taking 1 (off, the parent's seeded
selection) and 0 (the default) alternate step by step, so that drift hits both alike.  Every call
ends synchronised, so a host clock around it is the call's time.  The results of the two modes
are compared bitwise before anything is timed.  --warmup untimed steps of each mode, then --steps
timed ones: median, min and max of the call, of lrf_ms and of the setup and loop phases, and
se3icp_last_take_stats / se3icp_last_seed_stats / se3icp_last_graph_stats of the default mode.

C2's clouds are all distinct: nothing takes there, and its line is the unchanged path of the
changed kernel against itself, to be held against mode 1's own min-max spread.

Writes one JSON file (--out, default profiles/lrf_take_bench.json).
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


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def same(a, b):
    return (a.T.tobytes() == b.T.tobytes() and a.num_iterations == b.num_iterations and a.status == b.status
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.scaling_factor == b.scaling_factor)


def run_workload(se3icp, torch, name, pairs, method, params, steps, warmup):
    d_src = torch.from_numpy(np.concatenate([s for s, _ in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([t for _, t in pairs])).cuda()
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    to = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
    torch.cuda.synchronize()

    def call(mode):
        se3icp.set_lrf_taking(mode)
        t0 = time.perf_counter()
        res = se3icp.register_batch_device(d_src.data_ptr(), so, d_tgt.data_ptr(), to, method, params)
        return time.perf_counter() - t0, res, se3icp.last_kernel_times()

    out = dict(workload=name, method=method, pairs=len(pairs), points=int(so[-1] + to[-1]))
    try:
        _, want, k1 = call(1)
        _, got, k0 = call(0)
        out["take_stats"] = se3icp.last_take_stats()
        out["seed_stats"] = se3icp.last_seed_stats()
        out["graph_stats"] = se3icp.last_graph_stats()
        out["results_differing"] = sum(not same(a, b) for a, b in zip(got, want))
        out["iterations_total"] = sum(r.num_iterations for r in want)
        out["hand_overs"] = dict(mode_1=k1["lrf_fallback"], default=k0["lrf_fallback"])
        # k_lrf8's and k_lrf's work per call: leaf scans, bound tightenings / sorts, list candidates
        out["lrf_work"] = {name: {k: kt[k] for k in ("lrf_queries", "lrf_leaves", "lrf_merges", "lrf_candidates")}
                           for name, kt in (("mode_1", k1), ("default", k0))}
        for _ in range(warmup):
            call(1)
            call(0)
        keys = ("ms", "lrf_ms", "setup_ms", "loop_ms")
        acc = {m: {k: [] for k in keys} for m in (1, 0)}
        for _ in range(steps):
            for m in (1, 0):
                dt, res, kt = call(m)
                a = acc[m]
                a["ms"].append(dt * 1e3)
                a["lrf_ms"].append(kt["lrf_ms"])
                a["setup_ms"].append(res[0].time_setup_ms)
                a["loop_ms"].append(res[0].time_loop_ms)
    finally:
        se3icp.set_lrf_taking(0)
    out["mode_1"] = {k: med(v) for k, v in acc[1].items()}
    out["default"] = {k: med(v) for k, v in acc[0].items()}
    b, g = out["mode_1"]["ms"], out["default"]["ms"]
    out["ratio"] = g["median"] / b["median"]
    out["saved_ms"] = b["median"] - g["median"]
    # lrf_ms saved per taking class: the cost of a taken class is a seeded class's less this
    nt = out["take_stats"]["classes_taking"]
    out["lrf_saved_ms_per_taking_class"] = ((out["mode_1"]["lrf_ms"]["median"] - out["default"]["lrf_ms"]["median"]) / nt
                                            if nt else 0.0)
    # a gain: the default's slowest step beats mode 1's fastest by more than mode 1's spread;
    # no loss: the default's median within mode 1's spread of mode 1's median
    out["gain_beyond_spread"] = b["min"] - g["max"] > b["max"] - b["min"]
    out["within_mode_1_spread"] = g["median"] <= b["median"] + (b["max"] - b["min"])
    print(json.dumps(dict(workload=name, mode_1_ms=b, default_ms=g, lrf_ms=[out["mode_1"]["lrf_ms"], out["default"]["lrf_ms"]],
                          differ=out["results_differing"], take=out["take_stats"])), flush=True)
    del d_src, d_tgt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C4,shard8,C2,C3,C5")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lrf_take_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("lrf_take_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    import bench
    import se3icp
    from se3icp import _lib, registration
    se3icp.load()
    registration.set_nn_events(False)  # as bench.py's timed steps
    result = dict(tool="tools/lrf_take_bench.py", steps=args.steps, warmup=args.warmup,
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
                                                se3icp.default_params(**W["params"]), args.steps, args.warmup))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
