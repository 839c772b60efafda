#!/usr/bin/env python3
"""Cost of the registration report, on one GPU (not part of bench.py's headline).

se3icp_register_batch_device against se3icp_register_batch_report_device with the KITTI
driver's parameters over three workloads:

  bunny8   8 C2-like synthetic bunny problems (bench.py's C2 pairs, 41,670 points a cloud), se3_pt2pt
  shard8   an 8-pair KITTI-like shard (bench.py's C4 pairs 0..7, ~120k points a cloud), se3_gicp
  c4       the 64-pair C4 batch, se3_gicp

Per step, alternating so that drift hits all alike: the plain entry, the report entry with
the summary only, the report entry with per-point outputs into device buffers.  Every call
ends synchronised, so a host clock around it is the call's time.  --warmup untimed steps
(buffers, code objects), then --steps timed ones (default 7); medians with min / max.  The
report entries' results are compared bitwise with the plain entry's at these sizes before
anything is timed.

--parent-lib PATH: the plain entry is timed again with another build of libse3icp.so (the
parent commit's) on the same inputs, in fresh child processes that alternate with children
running this build (parent, this, parent, this): the plain path must not be slower than the
parent by more than the parent's own two runs differ.  The children also return a digest of
their results, which must be equal.

Writes one JSON file (--out, default profiles/report_bench.json).
"""
import argparse
import hashlib
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

METHODS = dict(bunny8="se3_pt2pt", shard8="se3_gicp", c4="se3_gicp")
LIMIT = 0.5  # max_correspondence_distance of the timed reports (caller's units)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def same(a, b):
    return (np.array_equal(a.T, b.T) and a.num_iterations == b.num_iterations and a.status == b.status
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.scaling_factor == b.scaling_factor)


def digest(res):
    h = hashlib.sha256()
    for r in res:
        h.update(r.T.tobytes())
        h.update(np.array([r.num_iterations, r.num_pure_se3_iterations, r.status], np.int64).tobytes())
    return h.hexdigest()


def upload(torch, pairs):
    d_src = torch.from_numpy(np.concatenate([s for s, _ in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([t for _, t in pairs])).cuda()
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    to = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
    torch.cuda.synchronize()
    return d_src, d_tgt, so, to


def load_pairs(path):
    z = np.load(path)
    n = int(z["n"])
    return [(z[f"s{k}"], z[f"t{k}"]) for k in range(n)]


def child(args):
    """Time the plain entry only, with whatever library SE3ICP_LIB names; one JSON line."""
    import torch
    if not torch.cuda.is_available():
        sys.exit("report_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    # plain ctypes on the entry both builds have (the package's loader binds this build's
    # whole surface, which the parent's library does not export)
    import ctypes as C
    from se3icp import _lib
    from se3icp.registration import _results
    L = C.CDLL(_lib.LIB_PATH)
    vp, i64p = C.c_void_p, C.POINTER(C.c_int64)
    L.se3icp_register_batch_device.argtypes = [C.c_int, C.c_int32, vp, i64p, vp, i64p, C.c_int, C.POINTER(_lib.Params),
                                               C.POINTER(_lib.Result), vp]
    L.se3icp_default_params.argtypes = [C.POINTER(_lib.Params)]
    prm = _lib.Params()
    L.se3icp_default_params(C.byref(prm))
    # se3icp.kitti_params(): examples/benchmark_kitti.cpp:133-148
    prm.estimated_overlap, prm.max_num_se3_iterations, prm.mse, prm.mse_switch_error = 0.7, 10, 1e-7, 5e-7
    prm.number_of_nn_for_LRF = 90
    pairs = load_pairs(args.pairs)
    n = len(pairs)
    d_src, d_tgt, so, to = upload(torch, pairs)
    c_so, c_to = (C.c_int64 * (n + 1))(*[int(x) for x in so]), (C.c_int64 * (n + 1))(*[int(x) for x in to])
    res = (_lib.Result * n)()
    ms = []
    for k in range(args.warmup + args.steps):
        t0 = time.perf_counter()
        rc = L.se3icp_register_batch_device(0, n, vp(d_src.data_ptr()), c_so, vp(d_tgt.data_ptr()), c_to,
                                            _lib.METHODS.index(args.method), C.byref(prm), res, None)
        if rc != 0:
            sys.exit(f"report_bench: register_batch_device returned {rc}")
        if k >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(ms=ms, digest=digest(_results(res, n)), lib=os.environ.get("SE3ICP_LIB", "default"))))


def run_child(pairs_path, method, steps, warmup, lib):
    env = dict(os.environ)
    if lib:
        env["SE3ICP_LIB"] = lib
    else:
        env.pop("SE3ICP_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pairs", pairs_path, "--method", method,
                          "--steps", str(steps), "--warmup", str(warmup)], env=env, capture_output=True, text=True,
                         timeout=240)
    if out.returncode != 0:
        sys.exit(f"report_bench: child failed ({out.returncode}): {out.stderr[-2000:]}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def run_workload(se3icp, torch, name, pairs, method, steps, warmup, parent_lib, tmp):
    n = len(pairs)
    d_src, d_tgt, so, to = upload(torch, pairs)
    prm = se3icp.kitti_params()
    d_idx = torch.full((int(so[-1]),), -1, dtype=torch.int32, device="cuda")
    d_dist = torch.zeros(int(so[-1]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    a = (d_src.data_ptr(), so, d_tgt.data_ptr(), to, method, prm)

    def plain():
        t0 = time.perf_counter()
        res = se3icp.register_batch_device(*a)
        return (time.perf_counter() - t0) * 1e3, res, None

    def summary():
        t0 = time.perf_counter()
        res, rep = se3icp.register_batch_report_device(*a, max_correspondence_distance=LIMIT)
        return (time.perf_counter() - t0) * 1e3, res, rep

    def per_point():
        t0 = time.perf_counter()
        res, rep = se3icp.register_batch_report_device(*a, max_correspondence_distance=LIMIT,
                                                       corr_idx_ptr=d_idx.data_ptr(), corr_dist_ptr=d_dist.data_ptr())
        return (time.perf_counter() - t0) * 1e3, res, rep

    modes = dict(plain=plain, report_summary=summary, report_per_point=per_point)
    out = dict(workload=name, method=method, pairs=n, points=int(so[-1] + to[-1]), max_correspondence_distance=LIMIT)
    # results first: bitwise, at the timed sizes
    _, want, _ = plain()
    _, got_s, rep = summary()
    _, got_p, _ = per_point()
    out["results_differing"] = dict(report_summary=sum(not same(x, y) for x, y in zip(got_s, want)),
                                    report_per_point=sum(not same(x, y) for x, y in zip(got_p, want)))
    out["iterations_total"] = sum(r.num_iterations for r in want)
    out["fitness"] = med([r.fitness for r in rep])
    out["loop_ms_plain"] = want[0].time_loop_ms
    for _ in range(max(0, warmup - 1)):
        for f in modes.values():
            f()
    ms = {k: [] for k in modes}
    loop = {k: [] for k in modes}
    for _ in range(steps):
        for k, f in modes.items():
            dt, res, _ = f()
            ms[k].append(dt)
            loop[k].append(res[0].time_loop_ms)
    base = statistics.median(ms["plain"])
    out["ms"] = {k: med(v) for k, v in ms.items()}
    out["time_loop_ms"] = {k: med(v) for k, v in loop.items()}  # (the report is outside it)
    out["report_cost_ms"] = {k: statistics.median(ms[k]) - base for k in ("report_summary", "report_per_point")}
    del d_src, d_tgt, d_idx, d_dist
    torch.cuda.empty_cache()
    if parent_lib:
        path = os.path.join(tmp, f"{name}.npz")
        np.savez(path, n=n, **{f"s{k}": s for k, (s, _) in enumerate(pairs)}, **{f"t{k}": t for k, (_, t) in enumerate(pairs)})
        runs = [run_child(path, method, steps, warmup, lib) for lib in (parent_lib, None, parent_lib, None)]
        os.remove(path)
        par = [statistics.median(r["ms"]) for r in (runs[0], runs[2])]
        cur = [statistics.median(r["ms"]) for r in (runs[1], runs[3])]
        spread = abs(par[0] - par[1])
        # the same over the pooled steps: the medians of all the parent's / this build's steps,
        # and the range of the parent's own steps
        par_steps, cur_steps = runs[0]["ms"] + runs[2]["ms"], runs[1]["ms"] + runs[3]["ms"]
        out["plain_vs_parent"] = dict(parent_ms=par, this_ms=cur, parent_spread_ms=spread,
                                      slower_by_ms=statistics.mean(cur) - statistics.mean(par),
                                      within_parent_spread=statistics.mean(cur) - statistics.mean(par) <= spread,
                                      pooled_parent_ms=med(par_steps), pooled_this_ms=med(cur_steps),
                                      pooled_slower_by_ms=statistics.median(cur_steps) - statistics.median(par_steps),
                                      parent_step_range_ms=max(par_steps) - min(par_steps),
                                      results_equal=len({r["digest"] for r in runs}) == 1,
                                      all_ms=[r["ms"] for r in runs])
    print(json.dumps(dict(workload=name, ms={k: statistics.median(v) for k, v in ms.items()},
                          differ=out["results_differing"], parent=out.get("plain_vs_parent", {}).get("slower_by_ms"))),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="bunny8,shard8,c4")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_bench.json"))
    ap.add_argument("--parent-lib", default="", help="libse3icp.so of the parent commit: time its plain entry too")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pairs", default="", help=argparse.SUPPRESS)
    ap.add_argument("--method", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    if not torch.cuda.is_available():
        sys.exit("report_bench: no GPU visible (this is a measurement: no fallback)")
    torch.cuda.init()
    import se3icp
    from bench import make_pairs
    se3icp.load()
    result = dict(tool="tools/report_bench.py", steps=args.steps, warmup=args.warmup,
                  device=torch.cuda.get_device_name(0), workloads=[])
    with tempfile.TemporaryDirectory() as tmp:
        for wl in args.workloads.split(","):
            if wl == "bunny8":
                pairs, _ = make_pairs("C2", 8, 0, 8, 1975)
            elif wl == "shard8":
                pairs, _ = make_pairs("C4", 64, 0, 8, 1975)
            elif wl == "c4":
                pairs, _ = make_pairs("C4", 64, 0, 64, 1975)
            else:
                sys.exit(f"unknown workload {wl}")
            result["workloads"].append(run_workload(se3icp, torch, wl, pairs, METHODS[wl], args.steps, args.warmup,
                                                    args.parent_lib, tmp))
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
    print(json.dumps(dict(written=args.out)))


if __name__ == "__main__":
    main()
