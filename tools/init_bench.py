#!/usr/bin/env python3
"""The initial pose per edge (se3icp_register_graph_init_device, se3icp_transform_device) on
bench.py's C4 scans: 65 KITTI-like scans of se3icp/datasets.py (~120k points each) resident in
HBM, registered as the 64-edge chain scan i+1 onto scan i with se3_gicp and the KITTI driver's
parameters, one MI355X.  Every edge carries a pose of about 1 m and 2 degrees of yaw: the
generator's odometry between the two scans, off by a degree of yaw and 5 cm.

Four measurements, each the median, min and max of --steps calls after --warmup untimed ones,
every call ending synchronised so that a host clock around it is the call's time:

  (a) the posed chain, this build against --parent-lib (a library of the parent commit, which
      has no initial pose): the parent's caller moves the 64 sources with torch (X @ R.T + t)
      into a second buffer and registers 129 clouds with register_graph_device, both inside the
      timed call; this build calls register_graph_device(init=...).  The two differ in the last
      bits of the moved sources (torch's matmul is not the pinned arithmetic), so the iteration
      totals are reported beside the times.
  (b) seeding across the poses of a cloud (se3icp_set_pose_seeding 0 against 1): lrf_ms, classes,
      classes seeded, classes seeded across poses, seed failures.
  (c) the plain chain, no pose, on both libraries: the two builds' ranges must overlap.
  (d) se3icp_transform_device on the 65 scans, out of place, against the floor of 48 B per point
      at the HBM peak (8.0 TB/s).

A library is chosen when the package is imported (SE3ICP_LIB), so every (library, round) is a
fresh worker process; the libraries alternate, --rounds rounds, and what a library cannot do is
left out of its worker.  The driver itself never touches the GPU.  Without --parent-lib only this
build is measured and (a) and (c) say so.

Writes one JSON file (--out, default profiles/init_bench.json).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "se3-icp_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_BYTES_PER_S = 8.0e12


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def rz(deg, t):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, -s, 0.0, t[0]], [s, c, 0.0, t[1]], [0.0, 0.0, 1.0, t[2]], [0.0, 0.0, 0.0, 1.0]])


def worker(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("init_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    import bench
    import se3icp
    from se3icp import _lib, registration
    L = se3icp.load()
    registration.set_nn_events(False)  # as bench.py's timed steps
    has_init = hasattr(L, "se3icp_init_version")
    W = bench.WORKLOADS["C4"]
    params = se3icp.default_params(**W["params"])
    z = np.load(args.scans_file)
    n = int(z["n"])
    scans = [z[f"s{k}"] for k in range(n)]
    init = [np.ascontiguousarray(z["init"][p]) for p in range(n - 1)]
    edges = se3icp.sequence_edges(n)
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in scans])]).astype(np.int64)
    n_pts = int(off[-1])
    dev = torch.device("cuda", 0)
    d_all = torch.empty((2 * n_pts, 3), dtype=torch.float64, device=dev)  # the scans, then room for moved sources
    d_all[:n_pts] = torch.from_numpy(np.concatenate(scans)).to(dev)
    torch.cuda.synchronize()
    out = dict(library=os.path.relpath(_lib.LIB_PATH, ROOT), has_init=has_init, device=torch.cuda.get_device_name(0),
               scans=n, points=n_pts)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ms, last = [], None
        for _ in range(args.steps):
            t0 = time.perf_counter()
            last = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, last

    def summary(ms, res):
        kt = se3icp.last_kernel_times()
        return dict(ms=med(ms), iterations_total=sum(r.num_iterations for r in res),
                    statuses_not_ok=sum(r.status != 0 for r in res), lrf_ms=kt["lrf_ms"],
                    setup_ms=res[0].time_setup_ms, loop_ms=res[0].time_loop_ms, graph_stats=se3icp.last_graph_stats())

    # (c) the plain chain
    ms, res = timed(lambda: se3icp.register_graph_device(d_all.data_ptr(), off, edges, W["method"], params))
    out["plain"] = summary(ms, res)

    # (a) the posed chain
    if has_init:
        ms, res = timed(lambda: se3icp.register_graph_device(d_all.data_ptr(), off, edges, W["method"], params, init=init))
        out["posed"] = dict(summary(ms, res), how="register_graph_device(init=...)", init_stats=se3icp.last_init_stats())
    else:
        Rt = [torch.from_numpy(np.ascontiguousarray(T[:3, :3].T)).to(dev) for T in init]
        tt = [torch.from_numpy(np.ascontiguousarray(T[:3, 3])).to(dev) for T in init]
        src_off = [int(off[s]) for s, _ in edges]
        src_n = [int(off[s + 1] - off[s]) for s, _ in edges]
        ext_off = np.concatenate([off, n_pts + np.cumsum(src_n)]).astype(np.int64)
        edges2 = [(n + p, t) for p, (_, t) in enumerate(edges)]
        torch.cuda.synchronize()

        def moved_chain():
            for p in range(len(edges)):
                a, m = src_off[p], src_n[p]
                b = int(ext_off[n + p])
                torch.addmm(tt[p], d_all[a:a + m], Rt[p], out=d_all[b:b + m])
            torch.cuda.synchronize()  # the engine's stream is not torch's
            return se3icp.register_graph_device(d_all.data_ptr(), ext_off, edges2, W["method"], params)

        ms, res = timed(moved_chain)
        out["posed"] = dict(summary(ms, res), how="torch X @ R.T + t into a second buffer, register_graph_device on "
                                                  f"{2 * n - 1} clouds")

    if has_init:
        # (b) seeding across the poses of a cloud: on and off alternate call by call
        acc = {0: dict(ms=[], lrf_ms=[]), 1: dict(ms=[], lrf_ms=[])}
        info = {}
        try:
            for step in range(args.warmup + args.steps):
                for mode in (0, 1):
                    se3icp.set_pose_seeding(mode)
                    t0 = time.perf_counter()
                    res = se3icp.register_graph_device(d_all.data_ptr(), off, edges, W["method"], params, init=init)
                    dt = (time.perf_counter() - t0) * 1e3
                    kt = se3icp.last_kernel_times()
                    if step >= args.warmup:
                        acc[mode]["ms"].append(dt)
                        acc[mode]["lrf_ms"].append(kt["lrf_ms"])
                    info[mode] = dict(classes=se3icp.last_graph_stats()["classes"], seed_stats=se3icp.last_seed_stats(),
                                      init_stats=se3icp.last_init_stats(), lrf_fallback=kt["lrf_fallback"],
                                      iterations_total=sum(r.num_iterations for r in res),
                                      T_bytes=hash(b"".join(r.T.tobytes() for r in res)))
        finally:
            se3icp.set_pose_seeding(0)
        out["seeding"] = {("on" if m == 0 else "off"): dict(ms=med(acc[m]["ms"]), lrf_ms=med(acc[m]["lrf_ms"]),
                                                             **{k: v for k, v in info[m].items() if k != "T_bytes"})
                          for m in (0, 1)}
        out["seeding"]["results_differ"] = int(info[0]["T_bytes"] != info[1]["T_bytes"])

        # (d) the transform stage, out of place
        poses = [np.eye(4)] + init
        dst = d_all.data_ptr() + 24 * n_pts
        ms, _ = timed(lambda: se3icp.transform_device(d_all.data_ptr(), off, poses, dst))
        m = med(ms)
        floor_ms = 48.0 * n_pts / HBM_PEAK_BYTES_PER_S * 1e3
        # the same on the GPU timeline: events on a torch stream around the call's work there (the
        # two table copies and the kernel), without the launch path and the wait
        ts = torch.cuda.Stream()  # (a stream of its own: the null stream would mean the engine's)
        gpu_ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(ts)
            se3icp.transform_device(d_all.data_ptr(), off, poses, dst, stream=ts.cuda_stream)
            e1.record(ts)
            e1.synchronize()
            gpu_ms.append(e0.elapsed_time(e1))
        g = med(gpu_ms)
        first = d_all[n_pts:n_pts + int(off[1])].cpu().numpy()
        out["transform"] = dict(ms=m, floor_ms=floor_ms, ratio_to_floor=m["median"] / floor_ms,
                                gpu_timeline_ms=g, gpu_timeline_ratio_to_floor=g["median"] / floor_ms,
                                gpu_timeline_GBps=48.0 * n_pts / (g["median"] * 1e-3) / 1e9,
                                GBps=48.0 * n_pts / (m["median"] * 1e-3) / 1e9,
                                note="a call's time on the host clock: launch, two table copies and one wait included",
                                first_scan_differs=int(first.tobytes() != se3icp.transform_points(poses[0], scans[0]).tobytes()))
    print("INIT_BENCH_WORKER " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scans", type=int, default=65)
    ap.add_argument("--n-az", type=int, default=1975)
    ap.add_argument("--parent-lib", default="", help="libse3icp.so of the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "init_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--scans-file", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    from se3icp import datasets, registration
    scans, poses = datasets.kitti_like_sequence(args.scans, seed=4, n_az=args.n_az)
    edges = registration.sequence_edges(args.scans)
    drift = rz(1.0, [0.05, 0.0, 0.0])
    init = [np.ascontiguousarray(drift @ M) for M in registration.edge_inits(poses, edges)]
    for M in init:
        M[3] = (0.0, 0.0, 0.0, 1.0)
    yaw = [float(np.rad2deg(np.arctan2(M[1, 0], M[0, 0]))) for M in init]
    step = [float(np.linalg.norm(M[:3, 3])) for M in init]
    this_lib = os.path.join(ROOT, "se3-icp_amd", "lib", "libse3icp.so")
    libs = ([("parent", os.path.abspath(args.parent_lib))] if args.parent_lib else []) + [("this", this_lib)]
    result = dict(tool="tools/init_bench.py", steps=args.steps, warmup=args.warmup, rounds=args.rounds, scans=args.scans,
                  hbm_peak_TBps=HBM_PEAK_BYTES_PER_S / 1e12,
                  pose=dict(yaw_deg=med([abs(y) for y in yaw]), translation_m=med(step)), runs=[])
    if not args.parent_lib:
        result["not_measured"] = "the parent's side of (a) and (c): no --parent-lib given"
    with tempfile.TemporaryDirectory() as tmp:
        f = os.path.join(tmp, "scans.npz")
        np.savez(f, n=args.scans, init=np.stack(init),
                 **{f"s{k}": np.ascontiguousarray(s, dtype=np.float64) for k, s in enumerate(scans)})
        for rnd in range(args.rounds):
            for name, lib in libs:
                env = dict(os.environ, SE3ICP_LIB=lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scans-file", f, "--steps", str(args.steps),
                       "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, env=env, capture_output=True, text=True)
                line = [ln for ln in p.stdout.splitlines() if ln.startswith("INIT_BENCH_WORKER ")]
                if p.returncode != 0 or not line:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    sys.exit(f"init_bench: the worker of {name} (round {rnd}) failed with {p.returncode}")
                run = dict(build=name, round=rnd, **json.loads(line[0][len("INIT_BENCH_WORKER "):]))
                result["runs"].append(run)
                print(json.dumps(dict(build=name, round=rnd, plain_ms=run["plain"]["ms"]["median"],
                                      posed_ms=run["posed"]["ms"]["median"],
                                      posed_iterations=run["posed"]["iterations_total"])), flush=True)
    # what the rounds say
    by = lambda name, key: [r[key]["ms"] for r in result["runs"] if r["build"] == name]
    verdict = {}
    for key in ("plain", "posed"):
        verdict[key] = {name: dict(median_of_medians=statistics.median(m["median"] for m in by(name, key)),
                                   min=min(m["min"] for m in by(name, key)), max=max(m["max"] for m in by(name, key)))
                        for name, _ in libs}
    if args.parent_lib:
        a, b = verdict["plain"]["parent"], verdict["plain"]["this"]
        verdict["plain_ranges_overlap"] = bool(a["min"] <= b["max"] and b["min"] <= a["max"])
    seeds = [r["seeding"] for r in result["runs"] if "seeding" in r]
    if seeds:
        verdict["seeding_lrf_ms_on_below_off_in_every_round"] = bool(
            all(s["on"]["lrf_ms"]["median"] < s["off"]["lrf_ms"]["median"] for s in seeds))
        verdict["seeding_lrf_ms"] = [dict(on=s["on"]["lrf_ms"]["median"], off=s["off"]["lrf_ms"]["median"]) for s in seeds]
    result["verdict"] = verdict
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(result, fo, indent=1)
    print(json.dumps(dict(written=args.out, verdict=verdict)))


if __name__ == "__main__":
    main()
