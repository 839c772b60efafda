#!/usr/bin/env python3
"""The voxel-grid downsample (se3icp_voxel_downsample_device) on bench.py's C4 scans: the 65
KITTI-like scans of se3icp/datasets.py (~120k points each), resident in HBM, all in one call.

Two voxel sizes, found by bisection on the first scan so that about 1/2 and about 1/10 of its
points remain.  For each: the call's time (every call ends synchronised, so a host clock around
it is the call's time; --warmup untimed calls, then the median, min and max of --steps timed
ones), the input rate in GB/s, the ratio to the floor "24 B read per point + 24 B written per
voxel at the HBM peak" (8.0 TB/s, the micro-architecture guide's figure for the MI355X), and
beside it the time of register_graph_device (bench.py's C4 method and parameters, the scans as a
sequence: scan i+1 onto scan i) on the call's output.  Before anything is timed the first scan's
slice of the batch output is compared bitwise with its lone downsample.

Writes one JSON file (--out, default profiles/voxel_bench.json).
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

HBM_PEAK_BYTES_PER_S = 8.0e12


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def voxel_for_fraction(se3icp, scan, fraction):
    """A voxel size that leaves about `fraction` of the scan's points (bisection in log space)."""
    lo, hi = 1e-3, 10.0
    n = scan.shape[0]
    for _ in range(24):
        mid = float(np.sqrt(lo * hi))
        if se3icp.voxel_downsample(scan, mid).shape[0] > fraction * n:
            lo = mid
        else:
            hi = mid
    return float(np.sqrt(lo * hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--graph-steps", type=int, default=3)
    ap.add_argument("--voxel-sizes", default="", help="two voxel sizes 'half,tenth' instead of the bisection "
                                                      "(a profiler run: only the timed calls' kernels)")
    ap.add_argument("--scans", type=int, default=65)
    ap.add_argument("--n-az", type=int, default=1975)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("voxel_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    import bench
    import se3icp
    from se3icp import _lib, datasets, registration
    se3icp.load()
    registration.set_nn_events(False)  # as bench.py's timed steps
    W = bench.WORKLOADS["C4"]
    params = se3icp.default_params(**W["params"])
    scans, _ = datasets.kitti_like_sequence(args.scans, seed=4, n_az=args.n_az)
    scans = [np.ascontiguousarray(s, dtype=np.float64) for s in scans]
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])])
    n_pts = int(off[-1])
    d_in = torch.from_numpy(np.concatenate(scans)).cuda()
    d_out = torch.empty_like(d_in)
    torch.cuda.synchronize()
    edges = se3icp.sequence_edges(len(scans))
    result = dict(tool="tools/voxel_bench.py", steps=args.steps, warmup=args.warmup, scans=len(scans), points=n_pts,
                  library=os.path.relpath(_lib.LIB_PATH, ROOT), device=torch.cuda.get_device_name(0),
                  hbm_peak_TBps=HBM_PEAK_BYTES_PER_S / 1e12, method=W["method"], cases=[])
    given = [float(x) for x in args.voxel_sizes.split(",") if x]
    for k, (name, fraction) in enumerate((("half", 0.5), ("tenth", 0.1))):
        v = given[k] if len(given) == 2 else voxel_for_fraction(se3icp, scans[0], fraction)
        lone = se3icp.voxel_downsample(scans[0], v)

        def call():
            t0 = time.perf_counter()
            oo = se3icp.voxel_downsample_device(d_in.data_ptr(), off, v, d_out.data_ptr())
            return (time.perf_counter() - t0) * 1e3, oo

        _, out_off = call()
        first = d_out[:out_off[1]].cpu().numpy()
        differ = int(first.shape != lone.shape or first.tobytes() != lone.tobytes())
        for _ in range(args.warmup):
            call()
        ms = [call()[0] for _ in range(args.steps)]
        n_out = int(out_off[-1])
        m = med(ms)
        floor_ms = (24.0 * n_pts + 24.0 * n_out) / HBM_PEAK_BYTES_PER_S * 1e3
        graph_ms, iters = [], 0
        for _ in range(args.graph_steps):
            call()  # (the registration reads the downsample's output: keep it the call's)
            t0 = time.perf_counter()
            res = se3icp.register_graph_device(d_out.data_ptr(), out_off, edges, W["method"], params)
            graph_ms.append((time.perf_counter() - t0) * 1e3)
            iters = sum(r.num_iterations for r in res)
        case = dict(case=name, voxel_size=v, points_out=n_out, fraction_out=n_out / n_pts,
                    first_scan_differs_from_lone=differ, ms=m, input_GBps=24.0 * n_pts / (m["median"] * 1e-3) / 1e9,
                    floor_ms=floor_ms, ratio_to_floor=m["median"] / floor_ms)
        if graph_ms:
            case.update(register_graph_device_ms=med(graph_ms), register_graph_iterations=iters,
                        downsample_share_of_both=m["median"] / (m["median"] + statistics.median(graph_ms)))
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
