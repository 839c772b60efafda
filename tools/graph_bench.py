#!/usr/bin/env python3
"""Registration over a shared cloud set against the expanded batch, on one GPU (not part of
bench.py's headline).

se3_gicp with the KITTI driver's parameters over three workloads of KITTI-like scans (bench.py's
C4 sequence, ~120k points a scan):

  shard8   scans 0..8, scan i+1 onto scan i: 8 edges, 16 uses of 9 clouds
  c4       scans 0..64, scan i+1 onto scan i: the 64-pair C4 batch, 128 uses of 65 clouds
  onemap   scans 0..8, every scan but scan 4 onto scan 4: 8 edges, the map used 8 times

Per step, in this order and alternating so that drift hits all alike:
se3icp_register_batch_device on the expanded pair list (the existing entry; its clouds are
concatenated per side in HBM, every shared scan twice), then se3icp_register_graph_device at
sharing 1, 2, 3 and 0 (the engine's choice) on the scans concatenated once.  Every call ends
synchronised, so a host clock around it is the call's time.  --warmup untimed steps, then
--steps timed ones; medians with min / max.  The graph's results are compared bitwise with the
batch's at these sizes before anything is timed.

--host times the host-buffer entries instead (every call uploads its clouds: the batch every
use, the graph every distinct cloud).  --plain times the existing entry alone (fresh process, the library SE3ICP_LIB names): the
same build's plain path against the parent commit's.

Writes one JSON file (--out, default profiles/graph_bench.json).
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

LEVELS = [1, 2, 3, 0]


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def same(a, b):
    return (a.T.tobytes() == b.T.tobytes() and a.num_iterations == b.num_iterations and a.status == b.status
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.scaling_factor == b.scaling_factor)


def run_workload(se3icp, torch, name, scans, edges, method, steps, warmup, plain_only, host=False):
    params = se3icp.kitti_params()
    used = sorted({c for e in edges for c in e})
    remap = {c: i for i, c in enumerate(used)}
    clouds = [scans[c] for c in used]
    edges = [(remap[s], remap[t]) for s, t in edges]
    pairs = [(clouds[a], clouds[b]) for a, b in edges]
    n = len(edges)
    d_src = torch.from_numpy(np.concatenate([s for s, _ in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([t for _, t in pairs])).cuda()
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    to = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
    d_all = torch.from_numpy(np.concatenate(clouds)).cuda()
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])])
    torch.cuda.synchronize()

    def batch():
        t0 = time.perf_counter()
        if host:
            res = se3icp.register_batch(pairs, method, params)
        else:
            res = se3icp.register_batch_device(d_src.data_ptr(), so, d_tgt.data_ptr(), to, method, params)
        return time.perf_counter() - t0, res, se3icp.last_kernel_times()

    def graph(lv):
        t0 = time.perf_counter()
        if host:
            res = se3icp.register_graph(clouds, edges, method, params, sharing=lv)
        else:
            res = se3icp.register_graph_device(d_all.data_ptr(), off, edges, method, params, sharing=lv)
        return time.perf_counter() - t0, res, se3icp.last_kernel_times()

    out = dict(workload=name, method=method, buffers="host" if host else "device", edges=n, clouds=len(clouds), points_distinct=int(off[-1]),
               points_uses=int(so[-1] + to[-1]), second_uses=2 * n - len(clouds))
    _, want, _ = batch()
    out["iterations_total"] = sum(r.num_iterations for r in want)
    if not plain_only:
        differ, stats = {}, {}
        for lv in LEVELS:
            _, got, _ = graph(lv)
            differ[str(lv)] = sum(not same(got[p], want[p]) for p in range(n))
            stats[str(lv)] = se3icp.last_graph_stats()
        out["results_differing"] = differ
        out["graph_stats"] = stats
    for _ in range(warmup):
        batch()
        if not plain_only:
            for lv in LEVELS:
                graph(lv)
    keys = ("ms", "lrf_ms", "setup_ms", "loop_ms")
    t_b = {k: [] for k in keys}
    t_g = {lv: {k: [] for k in keys} for lv in LEVELS}

    def note(acc, dt, res, kt):
        acc["ms"].append(dt * 1e3)
        acc["lrf_ms"].append(kt["lrf_ms"])
        acc["setup_ms"].append(res[0].time_setup_ms)
        acc["loop_ms"].append(res[0].time_loop_ms)

    for _ in range(steps):
        note(t_b, *batch())
        if not plain_only:
            for lv in LEVELS:
                note(t_g[lv], *graph(lv))
    out["batch"] = {k: med(v) for k, v in t_b.items()}
    line = dict(workload=name, batch_ms=out["batch"]["ms"]["median"])
    if not plain_only:
        b = out["batch"]["ms"]
        out["graph"] = {}
        for lv in LEVELS:
            g = {k: med(v) for k, v in t_g[lv].items()}
            g["ratio_to_batch"] = g["ms"]["median"] / b["median"]
            g["saved_ms"] = b["median"] - g["ms"]["median"]
            # the bar: not slower than the batch by more than the batch's own min-max spread
            g["within_batch_spread"] = g["ms"]["median"] <= b["median"] + (b["max"] - b["min"])
            out["graph"][str(lv)] = g
        line["graph_ms"] = {str(lv): out["graph"][str(lv)]["ms"]["median"] for lv in LEVELS}
        line["differ"] = out["results_differing"]
    print(json.dumps(line), flush=True)
    del d_src, d_tgt, d_all
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="shard8,c4,onemap")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n-az", type=int, default=1975)
    ap.add_argument("--scan-cache", default="", help="an .npz file for the generated scans (reused by later runs)")
    ap.add_argument("--plain", action="store_true", help="time se3icp_register_batch_device alone")
    ap.add_argument("--host", action="store_true", help="the host-buffer entries (se3icp_register_batch / "
                    "se3icp_register_graph: every call uploads its clouds) instead of the _device ones")
    ap.add_argument("--package-dir", default="", help="with --plain: import se3icp from here (another commit's "
                    "package with its own library, e.g. the parent's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("graph_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    if args.package_dir:
        sys.path.insert(0, os.path.abspath(args.package_dir))
    import se3icp
    from se3icp import datasets, _lib
    se3icp.load()
    wls = args.workloads.split(",")
    n_scans = 65 if "c4" in wls else 9
    if args.scan_cache and os.path.exists(args.scan_cache):
        z = np.load(args.scan_cache)
        scans = [z[f"s{k}"] for k in range(len(z.files))]
    else:
        scans, _ = datasets.kitti_like_sequence(65, seed=4, n_az=args.n_az, scan_indices=range(n_scans))
        scans = scans[:n_scans]
        if args.scan_cache:
            np.savez(args.scan_cache, **{f"s{k}": s for k, s in enumerate(scans)})
    assert len(scans) >= n_scans
    result = dict(tool="tools/graph_bench.py", steps=args.steps, warmup=args.warmup, plain_only=args.plain,
                  library=os.path.relpath(_lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0), workloads=[])
    for wl in wls:
        if wl == "shard8":
            edges = [(i + 1, i) for i in range(8)]
        elif wl == "c4":
            edges = [(i + 1, i) for i in range(64)]
        elif wl == "onemap":
            edges = [(i, 4) for i in range(9) if i != 4]
        else:
            sys.exit(f"unknown workload {wl}")
        result["workloads"].append(run_workload(se3icp, torch, wl, scans, edges, "se3_gicp", args.steps, args.warmup,
                                                args.plain, args.host))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
