"""GPU tests of the registration report (se3icp_register_*_report, k_report.hip).

The expected values are a numpy restatement of the definition in include/se3icp.h applied to
the engine's own returned T, in the caller's coordinates: for every source point the f64
nearest target point of T p (brute force, lowest index first, or scipy's cKDTree), its
distance, the inliers under the distance limit, and over them the long-double sums of G^T G.

Equality of indices and inlier sets is asserted with zero mismatches.  That needs inputs
without near-ties, and the tests assert that too, on the restatement: best and runner-up
distance differ by more than 1e-9 relative, and no distance lies within 1e-9 relative of the
limit.  The limits below (LIMITS) sit in gaps of the distance distribution found on the CPU
with the oracle's pose; each gap is more than 1e-6 relative wide.  The fixture is exempt by
construction: its 188 groups of duplicate target points test the tie rule.

Bounds (derived, not tuned; u = 2^-53):
  fitness      bitwise (one IEEE division of two integers); n_inliers exact.
  information  |GPU - long double| <= gamma sum |term| entry by entry, gamma =
               4 (depth + 3 + 8) u.  depth = 29 + ceil(blocks / 144) additions on the longest
               path of the order k_report / k_report_final build for a pair of `blocks` =
               ceil(n_src / 256) blocks: 6 halving steps of the wave sum, 2 for the block's
               four waves, ceil(blocks / 144) along one of the 18 x 8 chains, 3 to fold the
               eight chains, 18 for the last pass over the chunks (30 up to 36,864 points,
               31 up to 69,121).  3: the expansion of the moments (report.hpp); 8: the
               normalize / de-normalize round trip of a coordinate, squared; 4: the rounding
               of each two- or three-factor term.  An entry without terms must be 0 exactly.
  distances    |d_gpu - d_numpy| <= K u (|c_s| + |c_t| + radius), K = 68: 39 roundings of a
               coordinate-sized quantity -- centre subtraction and scale of both points (4),
               the engine's pose apply (6), difference (1), norm (6), unscale (1), the
               de-normalized translation t'/s - R c_s + c_t (8), numpy's pose apply (6),
               difference (1), norm (6) -- times sqrt(3) from components to the norm.
  inlier_rmse  the RMS is 1-Lipschitz in the largest per-point error, and its sum has the
               relative error gamma: |rmse_gpu - rmse_ld| <= K u (...) + gamma rmse_ld.
The observed maxima are recorded with parity_record (profiles/report_parity.json).
"""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
U53 = 2.0 ** -53
K_DIST = 68.0
UTM = np.array([4.5e5, 5.4e6, 300.0])


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


# ----------------------------------------------------------------------------- the restatement
def gamma(n_src):
    blocks = -(-n_src // 256)
    depth = 6 + 2 + -(-blocks // 144) + 3 + 18
    return 4.0 * (depth + 3 + 8) * U53


def nearest(q, tgt, brute):
    """(index, distance, runner-up distance) of every row of q among tgt, lowest index on ties."""
    if brute:
        j = np.empty(q.shape[0], np.int64)
        second = np.full(q.shape[0], np.inf)
        for a in range(0, q.shape[0], 256):
            d2 = ((q[a:a + 256, None, :] - tgt[None, :, :]) ** 2).sum(-1)
            j[a:a + 256] = d2.argmin(1)  # (the first minimum: the lowest index)
            if tgt.shape[0] > 1:
                second[a:a + 256] = np.sqrt(np.partition(d2, 1, axis=1)[:, 1])
    else:
        from scipy.spatial import cKDTree
        dd, jj = cKDTree(tgt).query(q, k=min(2, tgt.shape[0]))
        dd, jj = dd.reshape(q.shape[0], -1), jj.reshape(q.shape[0], -1)
        j = jj[:, 0]
        second = dd[:, 1] if dd.shape[1] > 1 else np.full(q.shape[0], np.inf)
    d = np.sqrt(((q - tgt[j]) ** 2).sum(1))
    return j, d, second


def all_inliers(max_d):
    return max_d <= 0 or max_d == math.inf


def restate(src, tgt, T, max_d, brute=False, ties_allowed=False):
    """The report of (src, tgt) at pose T by the definition, and the conditions under which
    the engine must agree with it index for index."""
    q = src @ T[:3, :3].T + T[:3, 3]
    j, d, second = nearest(q, tgt, brute)
    if not ties_allowed:
        assert ((second - d) > 1e-9 * second).all(), "near-tie in the restatement: the case is badly designed"
    inl = np.ones(d.shape[0], bool) if all_inliers(max_d) else d <= max_d
    if not all_inliers(max_d):
        assert (np.abs(d - max_d) > 1e-9 * max_d).all(), "a distance at the limit: the case is badly designed"
    x = tgt[j[inl]].astype(LD)
    n = int(inl.sum())
    info, mag = np.zeros((6, 6), LD), np.zeros((6, 6), LD)
    if n:
        S, Sa = x.sum(0), np.abs(x).sum(0)
        M = (x[:, :, None] * x[:, None, :]).sum(0)
        Ma = np.abs(x[:, :, None] * x[:, None, :]).sum(0)
        info[:3, :3] = np.trace(M) * np.eye(3, dtype=LD) - M
        mag[:3, :3] = Ma
        for a in range(3):
            mag[a, a] = Ma[(a + 1) % 3, (a + 1) % 3] + Ma[(a + 2) % 3, (a + 2) % 3]
        sk = np.array([[0, -S[2], S[1]], [S[2], 0, -S[0]], [-S[1], S[0], 0]], LD)
        ska = np.array([[0, Sa[2], Sa[1]], [Sa[2], 0, Sa[0]], [Sa[1], Sa[0], 0]], LD)
        info[:3, 3:], info[3:, :3] = sk, sk.T
        mag[:3, 3:], mag[3:, :3] = ska, ska.T
        info[3:, 3:] = mag[3:, 3:] = n * np.eye(3, dtype=LD)
    rmse = float(np.sqrt((d[inl].astype(LD) ** 2).sum() / n)) if n else 0.0
    cs, ct = src.mean(0), tgt.mean(0)
    radius = max(np.linalg.norm(src - cs, axis=1).max(), np.linalg.norm(tgt - ct, axis=1).max())
    eps_d = K_DIST * U53 * (np.linalg.norm(cs) + np.linalg.norm(ct) + radius)
    return dict(j=j.astype(np.int32), d=d, inl=inl, n=n, info=info, mag=mag, rmse=rmse, eps_d=eps_d)


def check_report(name, rep, want, n_src, parity_record):
    """One PairReport (with per-point arrays) against the restatement; returns the deviations."""
    g = gamma(n_src)
    assert rep.corr_idx is not None and rep.corr_idx.shape == (n_src,)
    mism = int((rep.corr_idx != want["j"]).sum())
    dev_d = float(np.abs(rep.corr_dist - want["d"]).max() / want["eps_d"])
    err = np.abs(rep.information.astype(LD) - want["info"])
    has = want["mag"] > 0
    dev_i = float((err[has] / (g * want["mag"][has])).max()) if has.any() else 0.0
    dev_r = abs(rep.inlier_rmse - want["rmse"]) / (want["eps_d"] + g * want["rmse"])
    print(f"[report] {name}: n_src {n_src} inliers {rep.n_inliers}/{want['n']} index mismatches {mism} "
          f"information {dev_i:.3f} of its bound, distances {dev_d:.3f}, rmse {dev_r:.3f}; "
          f"stop {rep.stop_reason_name} switched {rep.switched}")
    parity_record(f"report: {name}", n_src=n_src, n_inliers=want["n"], index_mismatches=mism,
                  information_over_bound=dev_i, distance_over_bound=dev_d, rmse_over_bound=float(dev_r))
    assert mism == 0
    assert rep.n_inliers == want["n"]
    assert rep.fitness == want["n"] / n_src  # bitwise: the one IEEE division
    assert (rep.information[~has] == 0.0).all()
    assert dev_i <= 1.0
    assert dev_d <= 1.0
    assert dev_r <= 1.0
    if want["n"] == 0:
        assert rep.inlier_rmse == 0.0 and not rep.information.any()


def same_result(a, b):
    return (np.array_equal(a.T, b.T) and a.num_iterations == b.num_iterations
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.status == b.status
            and a.scaling_factor == b.scaling_factor)


def same_report(a, b):
    ok = (a.fitness == b.fitness and a.inlier_rmse == b.inlier_rmse and np.array_equal(a.information, b.information)
          and a.final_mse == b.final_mse and a.final_mse_change == b.final_mse_change and a.n_inliers == b.n_inliers
          and a.switched == b.switched and a.stop_reason == b.stop_reason)
    for x, y in ((a.corr_idx, b.corr_idx), (a.corr_dist, b.corr_dist)):
        if x is not None and y is not None:
            ok = ok and np.array_equal(x, y)
    return ok


# ----------------------------------------------------------------------------- the cases
_CACHE = {}


def method_pair(bunny_unique, kind):
    """Noisy 2 % bunny subsamples, n_src != n_tgt, the source cropped to the 70 % of its points
    lowest along x; `pt2pt` at a UTM-sized offset."""
    key = ("method", kind)
    if key not in _CACHE:
        from se3icp import datasets
        seed = {"pt2pt": 11, "se3_gicp": 12, "se3_gicp_with_cf": 13, "se3_pure_pt2pt": 14}[kind]
        rng = np.random.default_rng(seed)
        base = bunny_unique * 50.0
        T = datasets.make_T(datasets.rot_3d(*rng.uniform(-0.1, 0.1, 3)), rng.uniform(-0.3, 0.3, 3))
        src = base[rng.random(base.shape[0]) < 0.02]
        src = src[src[:, 0] <= np.quantile(src[:, 0], 0.7)]
        tgt = datasets.transform(T, base)[rng.random(base.shape[0]) < 0.02]
        src = src + rng.normal(0, 0.02, src.shape)
        tgt = tgt + rng.normal(0, 0.02, tgt.shape)
        if kind == "pt2pt":
            src, tgt = src + UTM, tgt + UTM
        src, tgt = np.ascontiguousarray(src), np.ascontiguousarray(tgt)
        assert src.shape[0] != tgt.shape[0]
        src.setflags(write=False)
        tgt.setflags(write=False)
        _CACHE[key] = (src, tgt)
    return _CACHE[key]


def method_params(mod, kind):
    if kind == "pt2pt":
        return mod.default_params(estimated_overlap=0.7, max_num_iterations=30)
    return mod.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                              number_of_nn_for_LRF=30)


def sums_params(mod):
    return mod.default_params(max_num_iterations=3)


def node_pair(bunny_unique):
    """4096 x 4096: every leaf of both kd-trees is full."""
    if "node" not in _CACHE:
        from se3icp import datasets
        rng = np.random.default_rng(21)
        base = bunny_unique * 50.0
        T = datasets.make_T(datasets.rot_3d(0.05, -0.04, 0.06), [0.2, -0.1, 0.15])
        src = base[rng.permutation(base.shape[0])[:4096]] + rng.normal(0, 0.02, (4096, 3))
        tgt = datasets.transform(T, base[rng.permutation(base.shape[0])[:4096]]) + rng.normal(0, 0.02, (4096, 3))
        _CACHE["node"] = (np.ascontiguousarray(src), np.ascontiguousarray(tgt))
    return _CACHE["node"]


# Distance limits: the middle of the widest gap of the sorted distances around the 0.7
# quantile (the sums pairs: 0.5), found with nearest() above at refcpu.register's pose.  On
# the CPU, with that pose: relative gap widths 2.4e-4 .. 4.1e-2, the smallest relative margin
# between best and runner-up 1.0e-5 (the 4096 x 4096 pair), fitness 0.41 .. 0.80.
LIMITS = {
    "pt2pt": 0.2598506082592421,             # 488 x 703, gap 1.4e-2, fitness 0.713
    "se3_gicp": 0.29309242296313026,         # 469 x 685, gap 1.1e-2, fitness 0.704
    "se3_gicp_with_cf": 0.29225474172358945,  # 488 x 724, gap 1.1e-2, fitness 0.762
    "se3_pure_pt2pt": 0.2808751172837148,    # 487 x 700, gap 1.6e-2, fitness 0.682
    "node": 0.13608070251684262,             # gap 3.1e-3, fitness 0.797
    1: 0.0,                                  # (one point: no gap to sit in; everything is an inlier)
    255: 0.11610275078094934, 256: 0.11389776025583526, 257: 0.12447008024096706,
    32256: 0.1273851412832295, 32257: 0.11617667356977276, 36864: 0.12955358480522006,
    36865: 0.11587165980309522, 69120: 0.12445206783455562, 69121: 0.11702647775573177,
}


def run_case(mod, pairs, method, params, max_d, device=0):
    """(plain results, report results, reports) of one batch, the plain call first."""
    plain = mod.register_batch(pairs, method, params, device=device)
    res, rep = mod.register_batch_report(pairs, method, params, device=device, max_correspondence_distance=max_d,
                                         per_point=True)
    return plain, res, rep


# ----------------------------------------------------------------------------- 1: the fixture
def test_fixture(se3icp_mod, fixture_clouds, parity_record):
    """se3_pt2pl with the CLI parameters, no distance limit: everything is an inlier, and the
    target's duplicate points answer with the lowest index of their group."""
    src, tgt = fixture_clouds
    prm = se3icp_mod.cli_params()
    plain, res, rep = run_case(se3icp_mod, [(src, tgt)], "se3_pt2pl", prm, 0.0)
    assert same_result(plain[0], res[0])  # (6: the results are untouched)
    r = rep[0]
    assert r.fitness == 1.0 and r.n_inliers == 4167
    from se3icp import _lib
    assert r.stop_reason == _lib.STOP_CONVERGED and r.switched == 1
    # the tie rule: i -> the lowest index holding the same target point
    _, first, inv = np.unique(tgt, axis=0, return_index=True, return_inverse=True)
    lowest = first[inv.reshape(-1)]
    groups = np.bincount(inv.reshape(-1))
    assert int((groups > 1).sum()) == 188
    assert np.array_equal(r.corr_idx, lowest.astype(np.int32))
    want = restate(src, tgt, res[0].T, 0.0, brute=True, ties_allowed=True)
    check_report("fixture", r, want, 4167, parity_record)


# ----------------------------------------------------------------------------- 2: the kinds of method
@pytest.mark.parametrize("kind", ["pt2pt", "se3_gicp", "se3_gicp_with_cf", "se3_pure_pt2pt"])
def test_methods(se3icp_mod, bunny_unique, parity_record, kind):
    """Vanilla (raw frame, pivot at a UTM-sized offset), normalized, with confidences, and a
    pure SE(3) run whose loop never searched in R3; 0 < fitness < 1."""
    src, tgt = method_pair(bunny_unique, kind)
    plain, res, rep = run_case(se3icp_mod, [(src, tgt)], kind, method_params(se3icp_mod, kind), LIMITS[kind])
    assert same_result(plain[0], res[0])
    want = restate(src, tgt, res[0].T, LIMITS[kind], brute=True)
    check_report(kind, rep[0], want, src.shape[0], parity_record)
    assert 0 < rep[0].fitness < 1
    if kind == "se3_pure_pt2pt":
        assert res[0].num_pure_se3_iterations == res[0].num_iterations and rep[0].switched == 0


# ----------------------------------------------------------------------------- 3: the reduction's edges
def _sum_sizes():
    from test_gpu_loop import SUM_SIZES
    return SUM_SIZES


@pytest.mark.parametrize("n", _sum_sizes())
def test_reduction_edges(se3icp_mod, parity_record, n):
    """k_report_final copies k_reduce_final's layout (18 chunks x 8 chains over blocks of 256),
    so its order changes shape at SUM_SIZES: one thread, one block +- 1, 126|127, 144|145 and
    270|271 blocks."""
    from test_gpu_loop import sums_pair
    src, tgt = sums_pair(n)
    plain, res, rep = run_case(se3icp_mod, [(src, tgt)], "pt2pt", sums_params(se3icp_mod), LIMITS[n])
    assert same_result(plain[0], res[0])
    want = restate(src, tgt, res[0].T, LIMITS[n])
    check_report(f"sums n={n}", rep[0], want, n, parity_record)
    if n > 1:
        assert 0 < rep[0].fitness < 1


# ----------------------------------------------------------------------------- 4: full nodes
def test_full_local_node(se3icp_mod, bunny_unique, parity_record):
    src, tgt = node_pair(bunny_unique)
    prm = se3icp_mod.default_params(max_num_iterations=8)
    plain, res, rep = run_case(se3icp_mod, [(src, tgt)], "pt2pl", prm, LIMITS["node"])
    assert same_result(plain[0], res[0])
    want = restate(src, tgt, res[0].T, LIMITS["node"], brute=True)
    check_report("4096 x 4096", rep[0], want, 4096, parity_record)


# ----------------------------------------------------------------------------- 5: the limit's semantics
def test_distance_limit_semantics(se3icp_mod, bunny_unique, parity_record):
    src, tgt = method_pair(bunny_unique, "se3_gicp")
    prm = method_params(se3icp_mod, "se3_gicp")
    plain = se3icp_mod.register_batch([(src, tgt)], "se3_gicp", prm)
    reps = {}
    for d in (0.0, -1.0, math.inf, 1e-9):
        res, rep = se3icp_mod.register_batch_report([(src, tgt)], "se3_gicp", prm, max_correspondence_distance=d,
                                                    per_point=True)
        assert same_result(plain[0], res[0])
        reps[d] = rep[0]
    for d in (0.0, -1.0, math.inf):
        assert reps[d].fitness == 1.0 and reps[d].n_inliers == src.shape[0]
        assert same_report(reps[d], reps[0.0])
    check_report("no limit", reps[0.0], restate(src, tgt, plain[0].T, 0.0, brute=True), src.shape[0], parity_record)
    none = reps[1e-9]
    assert none.corr_dist.min() > 1e-9  # the limit is below the smallest distance
    assert none.n_inliers == 0 and none.fitness == 0.0 and none.inlier_rmse == 0.0
    assert not none.information.any()
    assert np.array_equal(none.corr_idx, reps[0.0].corr_idx) and np.array_equal(none.corr_dist, reps[0.0].corr_dist)


# ----------------------------------------------------------------------------- 7: batch independence
def five_pairs(bunny_unique):
    if "five" not in _CACHE:
        from se3icp import datasets
        out = []
        for seed, sub in ((31, 0.02), (32, 0.05), (33, 0.03), (34, 0.08), (35, 0.012)):
            s, t, _ = datasets.bunny_pair(bunny_unique, seed=seed, subsample=sub)
            out.append((s, t))
        _CACHE["five"] = out
    return _CACHE["five"]


FIVE_LIMIT = 0.12


@pytest.mark.parametrize("slot", [0, 1])
def test_batch_independence(se3icp_mod, bunny_unique, slot):
    """Five pairs of different sizes that finish at different iterations: every report field and
    per-point array of a pair in the batch is bitwise the pair's alone, on engine slots 0 and 1."""
    pairs = five_pairs(bunny_unique)
    prm = se3icp_mod.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                                    number_of_nn_for_LRF=30)
    dev = slot << 8
    res, rep = se3icp_mod.register_batch_report(pairs, "se3_pt2pl", prm, device=dev,
                                                max_correspondence_distance=FIVE_LIMIT, per_point=True)
    assert len({r.num_iterations for r in res}) > 1
    assert len({p[0].shape[0] for p in pairs}) == 5
    for k, pair in enumerate(pairs):
        r1, p1 = se3icp_mod.register_batch_report([pair], "se3_pt2pl", prm, device=dev,
                                                  max_correspondence_distance=FIVE_LIMIT, per_point=True)
        assert same_result(res[k], r1[0]), k
        assert same_report(rep[k], p1[0]), k
        assert rep[k].corr_idx.shape == (pair[0].shape[0],) and (rep[k].corr_idx >= 0).all()
    assert any(0 < r.fitness < 1 for r in rep)


# ----------------------------------------------------------------------------- 8: device outputs
def test_device_outputs(se3icp_mod, bunny_unique):
    import torch
    pairs = five_pairs(bunny_unique)[:3]
    prm = se3icp_mod.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                                    number_of_nn_for_LRF=30)
    host_res, host_rep = se3icp_mod.register_batch_report(pairs, "se3_gicp", prm, max_correspondence_distance=FIVE_LIMIT,
                                                          per_point=True)
    s_off = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in pairs])])
    t_off = np.concatenate([[0], np.cumsum([p[1].shape[0] for p in pairs])])
    d_src = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    d_idx = torch.full((int(s_off[-1]),), -1, dtype=torch.int32, device="cuda")
    d_dist = torch.zeros(int(s_off[-1]), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res, rep = se3icp_mod.register_batch_report_device(d_src.data_ptr(), s_off, d_tgt.data_ptr(), t_off, "se3_gicp", prm,
                                                       max_correspondence_distance=FIVE_LIMIT,
                                                       corr_idx_ptr=d_idx.data_ptr(), corr_dist_ptr=d_dist.data_ptr(),
                                                       outputs_on_device=True)
    idx, dist = d_idx.cpu().numpy(), d_dist.cpu().numpy()
    for k in range(len(pairs)):
        assert same_result(res[k], host_res[k]) and same_report(rep[k], host_rep[k]), k
        assert np.array_equal(idx[s_off[k]:s_off[k + 1]], host_rep[k].corr_idx), k
        assert np.array_equal(dist[s_off[k]:s_off[k + 1]], host_rep[k].corr_dist), k
    # and the summary alone, no per-point buffers
    res2, rep2 = se3icp_mod.register_batch_report_device(d_src.data_ptr(), s_off, d_tgt.data_ptr(), t_off, "se3_gicp",
                                                         prm, max_correspondence_distance=FIVE_LIMIT)
    assert all(same_result(a, b) and same_report(p, q) for a, b, p, q in zip(res2, host_res, rep2, host_rep))


# ----------------------------------------------------------------------------- 9: sweep
def test_sweep(se3icp_mod, bunny_unique):
    """Three alpha_rot variants with max_group = 2: two groups, the first with a replica."""
    pairs = five_pairs(bunny_unique)[:2]
    base = se3icp_mod.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                                     number_of_nn_for_LRF=30)
    variants = se3icp_mod.sweep_params(base, alpha_rot=[0.5, 3.0, 10.0])
    res, rep = se3icp_mod.register_sweep_report(pairs, "se3_pt2pl", variants, max_group=2,
                                                max_correspondence_distance=FIVE_LIMIT)
    plain = se3icp_mod.register_sweep(pairs, "se3_pt2pl", variants, max_group=2)
    for v, prm in enumerate(variants):
        r1, p1 = se3icp_mod.register_batch_report(pairs, "se3_pt2pl", prm, max_correspondence_distance=FIVE_LIMIT)
        for p in range(len(pairs)):
            assert same_result(res[v][p], plain[v][p]), (v, p)
            assert same_result(res[v][p], r1[p]), (v, p)
            assert same_report(rep[v][p], p1[p]), (v, p)
    # the device entry returns the same
    import torch
    s_off = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in pairs])])
    t_off = np.concatenate([[0], np.cumsum([p[1].shape[0] for p in pairs])])
    d_src = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
    d_tgt = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
    torch.cuda.synchronize()
    res_d, rep_d = se3icp_mod.register_sweep_report_device(d_src.data_ptr(), s_off, d_tgt.data_ptr(), t_off, "se3_pt2pl",
                                                           variants, max_group=2,
                                                           max_correspondence_distance=FIVE_LIMIT)
    for v in range(3):
        for p in range(len(pairs)):
            assert same_result(res_d[v][p], res[v][p]) and same_report(rep_d[v][p], rep[v][p]), (v, p)


# ----------------------------------------------------------------------------- 10: hygiene
def test_report_plain_report_sequence(se3icp_mod, bunny_unique):
    """A report call, a plain call and a report call of another batch size on one engine: each
    equals the same call on an engine slot nothing else has used."""
    pairs = five_pairs(bunny_unique)
    prm = se3icp_mod.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                                    number_of_nn_for_LRF=30)
    kw = dict(max_correspondence_distance=FIVE_LIMIT, per_point=True)
    a = se3icp_mod.register_batch_report(pairs[:3], "se3_pt2pl", prm, device=0, **kw)
    b = se3icp_mod.register_batch(pairs[:3], "se3_pt2pl", prm, device=0)
    c = se3icp_mod.register_batch_report(pairs[1:], "se3_pt2pl", prm, device=0, **kw)
    a_f = se3icp_mod.register_batch_report(pairs[:3], "se3_pt2pl", prm, device=5 << 8, **kw)
    b_f = se3icp_mod.register_batch(pairs[:3], "se3_pt2pl", prm, device=6 << 8)
    c_f = se3icp_mod.register_batch_report(pairs[1:], "se3_pt2pl", prm, device=7 << 8, **kw)
    for got, fresh in ((a, a_f), (c, c_f)):
        assert all(same_result(x, y) for x, y in zip(got[0], fresh[0]))
        assert all(same_report(x, y) for x, y in zip(got[1], fresh[1]))
    assert all(same_result(x, y) for x, y in zip(b, b_f))
    assert all(same_result(x, y) for x, y in zip(b, a[0]))


def _traced(mod, pairs, method, prm, report, pair=0, max_iters=160):
    """register_batch(_report) with the trace of one pair armed."""
    from se3icp import _lib
    L = _lib.load()
    ns = pairs[pair][0].shape[0]
    tr = {"corr_idx": np.full((max_iters, ns), -1, np.int32), "corr_dist": np.zeros((max_iters, ns), np.float32),
          "trim_key": np.zeros(max_iters, np.uint64), "T": np.zeros((max_iters, 4, 4)), "mse": np.zeros(max_iters),
          "phase": np.zeros(max_iters, np.int32)}
    t = _lib.Trace(pair, max_iters, tr["corr_idx"].ctypes.data_as(C.POINTER(C.c_int32)),
                   tr["corr_dist"].ctypes.data_as(C.POINTER(C.c_float)),
                   tr["trim_key"].ctypes.data_as(C.POINTER(C.c_uint64)), tr["T"].ctypes.data_as(C.POINTER(C.c_double)),
                   tr["mse"].ctypes.data_as(C.POINTER(C.c_double)), tr["phase"].ctypes.data_as(C.POINTER(C.c_int32)),
                   0, 0)
    _lib.check(L.se3icp_set_trace(0, C.byref(t)), "set_trace")
    try:
        if report:
            out = mod.register_batch_report(pairs, method, prm, max_correspondence_distance=FIVE_LIMIT, per_point=True)
        else:
            out = (mod.register_batch(pairs, method, prm), None)
    finally:
        L.se3icp_set_trace(0, None)
    n = int(t.iters_recorded)
    return out, n, {k: v[:n] for k, v in tr.items()}


def test_trace_records_the_loop_only(se3icp_mod, bunny_unique):
    """The report's search is not an iteration: an armed trace records what it records
    without the report."""
    pairs = five_pairs(bunny_unique)[:2]
    prm = se3icp_mod.default_params(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                                    number_of_nn_for_LRF=30)
    (res_r, rep_r), n_r, tr_r = _traced(se3icp_mod, pairs, "se3_pt2pl", prm, True, pair=1)
    (res_p, _), n_p, tr_p = _traced(se3icp_mod, pairs, "se3_pt2pl", prm, False, pair=1)
    assert n_r == n_p == res_r[1].num_iterations
    for k in tr_r:
        assert np.array_equal(tr_r[k], tr_p[k]), k
    assert all(same_result(a, b) for a, b in zip(res_r, res_p))
    untraced = se3icp_mod.register_batch_report(pairs, "se3_pt2pl", prm, max_correspondence_distance=FIVE_LIMIT,
                                                per_point=True)
    assert all(same_report(a, b) for a, b in zip(rep_r, untraced[1]))


# ----------------------------------------------------------------------------- 11: stop reasons
def test_stop_reasons_on_the_engine(se3icp_mod, bunny_unique):
    from se3icp import _lib
    pair = five_pairs(bunny_unique)[0]
    base = dict(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-9, mse_switch_error=0.0,
                number_of_nn_for_LRF=30)

    def run(method, **over):
        prm = se3icp_mod.default_params(**{**base, **over})
        res, rep = se3icp_mod.register_batch_report([pair], method, prm)
        return res[0], rep[0]

    # mse_switch_error = 0: the switch happens at max_num_se3_iterations = 10, and with
    # mse = 1e-9 the R3 phase is still moving at iteration 11
    res, rep = run("se3_pt2pl", max_num_iterations=11)
    assert res.num_iterations == 11 and res.num_pure_se3_iterations == 10
    assert rep.stop_reason == _lib.STOP_MAX_ITERATIONS and rep.switched == 1
    # a cap of 4 or 10 is passed by in the SE(3) phase: the run ends on its criterion
    for cap in (4, 10):
        res, rep = run("se3_pt2pl", max_num_iterations=cap, mse=1e-5)
        assert res.num_pure_se3_iterations == 10 and res.num_iterations > 10
        assert rep.stop_reason == _lib.STOP_CONVERGED and rep.switched == 1
    res, rep = run("se3_pure_pt2pt", max_num_se3_iterations=3)
    assert res.num_iterations == 3
    assert rep.stop_reason == _lib.STOP_MAX_SE3_ITERATIONS and rep.switched == 0
    assert rep.final_mse_change == abs(rep.final_mse_change) and np.isfinite(rep.final_mse)
