"""GPU tests of the initial pose per edge (se3icp_register_graph_init, se3icp_transform_device,
se3icp_set_initial_transform).

The contract needs no tolerance: with init[p] = T0, result p is bitwise what the plain entry
returns for (X', target), X' = apply_pose(T0, X), except T, which is compose(T_plain, T0).  So
every comparison is on the bytes of T plus num_iterations, num_pure_se3_iterations, status and
scaling_factor, against the plain entries of the same build on clouds moved by a numpy
restatement of apply_pose (csrc/pose.hpp: every product and sum rounded on its own, no FMA), the
expected T formed by a numpy restatement of compose.

Inputs:
  S     datasets.kitti_like_sequence(5, seed=4, n_az=200): ~12.5k points a scan
  B     four bunny clouds of 3,001 .. 3,544 points (test_gpu_graph.py's recipe)
  the fixture pair of tests/golden

Seed failures (se3icp_last_seed_stats' fourth value) of the posed chain are recorded through
parity_record, not asserted: a seed that rounding made too tight costs a trip to the exact
kernel and never a result.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = (1, 2, 3)


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


@pytest.fixture(scope="module")
def scans():
    from se3icp import datasets
    s, _ = datasets.kitti_like_sequence(5, seed=4, n_az=200)
    return [np.ascontiguousarray(x, dtype=np.float64) for x in s]


@pytest.fixture(scope="module")
def bunny_clouds(bunny_unique):
    from se3icp import datasets
    out = []
    for seed in (2, 3):
        src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=seed, subsample=0.1)
        out += [src, tgt]
    out[2] = out[2][:3001].copy()
    return [np.ascontiguousarray(c, dtype=np.float64) for c in out]


# ------------------------------------------------------------------ the restatement
def np_apply(T, X):
    """apply_pose of csrc/pose.hpp in numpy: one rounded operation per ufunc call."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty_like(X)
    p0, p1, p2 = X[:, 0], X[:, 1], X[:, 2]
    for e in range(3):
        out[:, e] = ((T[e, 0] * p0 + T[e, 1] * p1) + T[e, 2] * p2) + T[e, 3] * 1.0
    return np.ascontiguousarray(out)


def np_compose(A, B):
    """compose of csrc/pose.hpp in numpy scalars."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    C = np.zeros((4, 4))
    for i in range(3):
        for j in range(4):
            C[i, j] = ((A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]) + A[i, 3] * B[3, j]
    C[3, 3] = 1.0
    return C


def rigid(roll, pitch, yaw, t):
    from se3icp import datasets
    return np.ascontiguousarray(datasets.make_T(datasets.rot_3d(roll, pitch, yaw), t))


def odometry(k):
    """A guess of about 1 m and 2 degrees of yaw, different for every k."""
    return rigid(0.002 * (k + 1), -0.003 * (k + 1), np.deg2rad(2.0 - 0.5 * k), [1.0 - 0.1 * k, 0.05 * (k + 1), 0.01 * k])


def _bytes(r, T=None):
    return ((r.T if T is None else T).tobytes(), r.num_iterations, r.num_pure_se3_iterations, r.status,
            np.float64(r.scaling_factor).tobytes())


def _is_posed(T):
    return T is not None and T.tobytes() != np.eye(4).tobytes()


def moved_problem(clouds, edges, init):
    """The plain problem a posed one must equal: the cloud list extended by the numpy-made X' of
    every distinct (source, pose bits), in order of first use, and the edges redirected to them."""
    ext, seen, edges2 = list(clouds), {}, []
    for (s, t), T0 in zip(edges, init):
        if not _is_posed(T0):
            edges2.append((s, t))
            continue
        key = (s, T0.tobytes())
        if key not in seen:
            seen[key] = len(ext)
            ext.append(np_apply(T0, clouds[s]))
        edges2.append((seen[key], t))
    return ext, edges2, len(seen)


def check_posed(mod, parity_record, name, clouds, edges, init, method, params, levels=LEVELS):
    ext, edges2, n_var = moved_problem(clouds, edges, init)
    used = {c for e in edges for c in e}
    for lv in levels:
        got = mod.register_graph(clouds, edges, method, params, sharing=lv, init=init)
        st, ist = mod.last_graph_stats(), mod.last_init_stats()
        want = mod.register_graph(ext, edges2, method, params, sharing=lv)
        bad = []
        for p, T0 in enumerate(init):
            T = np_compose(want[p].T, T0) if _is_posed(T0) else want[p].T
            if _bytes(got[p]) != _bytes(want[p], T):
                bad.append(p)
        print(f"[init] {name} {method} sharing {lv}: {len(edges)} edges, {len(bad)} differ; {st}; {ist}")
        parity_record(f"init: {name} {method} sharing {lv}", edges=len(edges), differ=len(bad), **ist)
        assert not bad, [(p, got[p], want[p]) for p in bad[:2]]
        assert all(r.status == 0 for r in got)
        assert st["uses"] == 2 * len(edges)
        assert st["clouds"] == len(used)
        assert st["bytes_uploaded"] == 24 * sum(clouds[c].shape[0] for c in used)
        assert ist["posed_edges"] == sum(_is_posed(T0) for T0 in init)
        assert ist["posed_variants"] == n_var


# ------------------------------------------------------------------ 1. the transform stage
def _transform(mod, torch, clouds, poses, in_place, device=0):
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    dev = torch.device("cuda", 0)
    buf = torch.from_numpy(np.concatenate(clouds)).to(dev)
    out = buf if in_place else torch.full_like(buf, np.nan)
    torch.cuda.synchronize(dev)
    mod.transform_device(buf.data_ptr(), off, poses, None if in_place else out.data_ptr(), device=device)
    torch.cuda.synchronize(dev)
    got = out.cpu().numpy()
    if not in_place:
        assert np.array_equal(buf.cpu().numpy(), np.concatenate(clouds))  # the input is left alone
    return [got[off[c]:off[c + 1]] for c in range(len(clouds))]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4097])
def test_transform_device_sizes(se3icp_mod, n):
    import torch
    rng = np.random.default_rng(n)
    X = rng.normal(0.0, 30.0, (n, 3))
    T = rigid(0.3, -0.2, 1.1, [4.0, -5.0, 6.0])
    for in_place in (False, True):
        got = _transform(se3icp_mod, torch, [X], [T], in_place)[0]
        assert got.tobytes() == np_apply(T, X).tobytes(), (n, in_place)
    assert se3icp_mod.transform_points(T, X).tobytes() == np_apply(T, X).tobytes()


def test_transform_device_five_clouds(se3icp_mod):
    """Five clouds of different sizes in one launch (odd sizes: a cloud's first row is 8-B aligned
    only), a pose each, out of place, in place and on engine slot 1."""
    import torch
    rng = np.random.default_rng(5)
    sizes = [1025, 1, 3001, 64, 2049]
    clouds = [rng.normal(0.0, 50.0, (n, 3)) + 1e6 * (k == 2) for k, n in enumerate(sizes)]
    poses = [odometry(k) for k in range(5)]
    poses[3] = np.eye(4)
    want = [np_apply(T, X) for T, X in zip(poses, clouds)]
    for in_place, device in ((False, 0), (True, 0), (False, 1 << 8), (True, 1 << 8)):
        got = _transform(se3icp_mod, torch, clouds, poses, in_place, device)
        for k in range(5):
            assert got[k].tobytes() == want[k].tobytes(), (k, in_place, device)


# ------------------------------------------------------------------ 2. posed graph against the plain graph on X'
METHODS = ["se3_pt2pt", "se3_pt2pl", "se3_gicp", "gicp", "se3_pure_pt2pt"]


def _edge_sets(mod):
    I = np.eye(4)
    return {
        "chain all": (mod.sequence_edges(5), [odometry(k) for k in range(4)]),
        "chain every second": (mod.sequence_edges(5), [odometry(0), None, odometry(2), None]),
        # one cloud the source of three edges under two poses and the identity; the first pose twice
        "fan": ([(2, 1), (2, 3), (2, 0), (2, 3)], [odometry(0), odometry(1), I, odometry(0)]),
        "self": ([(1, 1), (2, 1)], [odometry(3), None]),
    }


@pytest.mark.parametrize("name", ["chain all", "chain every second", "fan", "self"])
@pytest.mark.parametrize("method", METHODS)
def test_posed_graph_on_scans(se3icp_mod, scans, parity_record, method, name):
    edges, init = _edge_sets(se3icp_mod)[name]
    check_posed(se3icp_mod, parity_record, f"S {name}", scans, edges, init, method, se3icp_mod.kitti_params())


@pytest.mark.parametrize("method", METHODS)
def test_posed_graph_mixed_sizes(se3icp_mod, bunny_clouds, parity_record, method):
    edges = [(0, 1), (2, 3), (1, 2), (3, 0), (0, 3)]
    small = [rigid(0.01 * (k + 1), -0.02, 0.015 * (k + 1), [0.002 * k, -0.001, 0.003]) for k in range(5)]
    init = [small[0], None, small[2], small[3], small[0]]
    check_posed(se3icp_mod, parity_record, "B mixed", bunny_clouds, edges, init, method, se3icp_mod.default_params())


# ------------------------------------------------------------------ 3. the device entry
def test_device_entry(se3icp_mod, scans):
    import torch
    mod = se3icp_mod
    edges, init = _edge_sets(mod)["chain every second"]
    params = mod.kitti_params()
    host = mod.register_graph(scans, edges, "se3_gicp", params, init=init)
    dev = torch.device("cuda", 0)
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in scans])]).astype(np.int64)
    buf = torch.from_numpy(np.concatenate(scans)).to(dev)
    torch.cuda.synchronize(dev)
    got = mod.register_graph_device(buf.data_ptr(), off, edges, "se3_gicp", params, init=init)
    assert mod.last_graph_stats()["bytes_uploaded"] == 0
    assert [_bytes(r) for r in got] == [_bytes(r) for r in host]
    # the plain device entry on what transform_device makes of the sources in HBM
    posed = [p for p, T0 in enumerate(init) if _is_posed(T0)]
    moved = [scans[edges[p][0]] for p in posed]
    ext_off = np.concatenate([off, off[-1] + np.cumsum([m.shape[0] for m in moved])]).astype(np.int64)
    ext = torch.from_numpy(np.concatenate(scans + moved)).to(dev)
    torch.cuda.synchronize(dev)
    tail = ext.data_ptr() + 24 * int(off[-1])
    mod.transform_device(tail, ext_off[len(scans):] - off[-1], [init[p] for p in posed])
    edges2 = list(edges)
    for k, p in enumerate(posed):
        edges2[p] = (len(scans) + k, edges[p][1])
    plain = mod.register_graph_device(ext.data_ptr(), ext_off, edges2, "se3_gicp", params)
    for p, T0 in enumerate(init):
        T = np_compose(plain[p].T, T0) if _is_posed(T0) else plain[p].T
        assert _bytes(got[p]) == _bytes(plain[p], T), p


def test_voxel_path_passes_the_pose_through(se3icp_mod, scans):
    """register_sequence(voxel_size=, init=): the raw scans downsampled in HBM, then the posed
    device entry -- bitwise register_graph(init=) on the clouds voxel_downsample returns."""
    mod = se3icp_mod
    edges, init = _edge_sets(mod)["chain every second"]
    params = mod.kitti_params()
    down = [mod.voxel_downsample(s, 0.5) for s in scans]
    want = mod.register_graph(down, edges, "se3_gicp", params, init=init)
    got = mod.register_sequence(scans, "se3_gicp", params, voxel_size=0.5, init=init)
    assert mod.last_init_stats()["posed_edges"] == 2
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want]


# ------------------------------------------------------------------ 4. reports
def _report_bytes(q):
    return (np.float64(q.fitness).tobytes(), np.float64(q.inlier_rmse).tobytes(), q.information.tobytes(),
            np.float64(q.final_mse).tobytes(), np.float64(q.final_mse_change).tobytes(), q.n_inliers, q.switched,
            q.stop_reason, q.corr_idx.tobytes(), q.corr_dist.tobytes())


@pytest.mark.parametrize("method", ["se3_gicp", "pt2pl"])
def test_reports(se3icp_mod, scans, method):
    mod = se3icp_mod
    edges, init = _edge_sets(mod)["fan"]
    params = mod.kitti_params()
    ext, edges2, _ = moved_problem(scans, edges, init)
    got, grep = mod.register_graph_report(scans, edges, method, params, max_correspondence_distance=0.5, per_point=True,
                                          init=init)
    want, wrep = mod.register_graph_report(ext, edges2, method, params, max_correspondence_distance=0.5, per_point=True)
    plain = mod.register_graph(scans, edges, method, params, init=init)
    for p, T0 in enumerate(init):
        T = np_compose(want[p].T, T0) if _is_posed(T0) else want[p].T
        assert _bytes(got[p]) == _bytes(want[p], T) == _bytes(plain[p]), p
        assert _report_bytes(grep[p]) == _report_bytes(wrep[p]), p
        assert grep[p].n_inliers > 0


# ------------------------------------------------------------------ 5. the object surface
def test_object_surface(se3icp_mod, fixture_clouds):
    mod = se3icp_mod
    src, tgt = fixture_clouds
    T0 = rigid(0.05, -0.04, 0.06, [0.1, -0.2, 0.05])
    want = mod.register_graph([src, tgt], [(0, 1)], "se3_pt2pl", None, init=[T0])[0]
    reg = mod.IterativeSE3Registration()
    reg.setSourceCloud(src)
    reg.setTargetCloud(tgt)
    reg.setInitialTransform(T0)
    reg.request_report(0.0, per_point=True)
    reg.run_se3_icp("pt2pl")
    assert (reg.current_estimated_T_.tobytes(), reg.num_iterations_, reg.num_pure_se3_iterations_, reg.status) == \
        (want.T.tobytes(), want.num_iterations, want.num_pure_se3_iterations, want.status)
    moved = mod.register_batch_report([(np_apply(T0, src), tgt)], "se3_pt2pl", None, per_point=True)
    assert want.T.tobytes() == np_compose(moved[0][0].T, T0).tobytes()
    assert _report_bytes(reg.report) == _report_bytes(moved[1][0])
    # cleared: the plain run
    reg2 = mod.IterativeSE3Registration()
    reg2.setSourceCloud(src)
    reg2.setTargetCloud(tgt)
    reg2.setInitialTransform(T0)
    reg2.setInitialTransform(None)
    reg2.run_se3_icp("pt2pl")
    assert reg2.current_estimated_T_.tobytes() == mod.register_batch([(src, tgt)], "se3_pt2pl")[0].T.tobytes()
    # through register_batch(init=)
    assert _bytes(mod.register_batch([(src, tgt)], "se3_pt2pl", init=[T0])[0]) == _bytes(want)


# ------------------------------------------------------------------ 6. seeding across variants
def test_seeding_across_variants(se3icp_mod, scans, parity_record):
    mod = se3icp_mod
    edges, init = _edge_sets(mod)["chain all"]
    params = mod.kitti_params()
    runs = {}
    try:
        for pose_mode, lrf_mode in ((0, 0), (1, 0), (0, 1), (0, 2), (0, 3)):
            mod.set_pose_seeding(pose_mode)
            mod.set_lrf_seeding(lrf_mode)
            res = mod.register_graph(scans, edges, "se3_gicp", params, sharing=2, init=init)
            runs[(pose_mode, lrf_mode)] = ([_bytes(r) for r in res], mod.last_init_stats(), mod.last_seed_stats(),
                                           mod.last_graph_stats())
    finally:
        mod.set_pose_seeding(0)
        mod.set_lrf_seeding(0)
    base = runs[(0, 0)]
    for key, (b, ist, sst, gst) in runs.items():
        print(f"[init] seeding pose {key[0]} lrf {key[1]}: {ist} {sst} classes {gst['classes']}")
        parity_record(f"init: seeding pose_mode={key[0]} lrf_mode={key[1]}", classes=gst["classes"], **ist, **sst)
        assert b == base[0], key
    assert runs[(0, 0)][1]["classes_seeded_across"] >= 1
    assert runs[(0, 0)][2]["classes_seeded"] >= runs[(0, 0)][1]["classes_seeded_across"]
    assert runs[(1, 0)][1]["classes_seeded_across"] == 0
    assert runs[(0, 1)][1]["classes_seeded_across"] == 0 and runs[(0, 1)][2]["classes_seeded"] == 0
    assert runs[(0, 2)][2]["queries_failed"] > 0  # halved seeds: the certificate fails, the results hold


def test_seeding_at_utm_offsets(se3icp_mod, parity_record):
    """Where the coordinate rounding of a pose is largest against the neighbour distances: 20,000
    points at UTM offsets (test_gpu_voxel.py's utm_cloud), turned about their own position.  The
    posed copy's selection starts from the raw cloud's distances; results are bitwise those without
    seeding, and the seeds that rounding made too tight are recorded."""
    mod = se3icp_mod
    rng = np.random.default_rng(12)
    at = np.array([5.1e5, 5.4e6, 300.0])
    A = at + rng.uniform(-40.0, 40.0, size=(20000, 3))
    B = np.ascontiguousarray(A[::2] + rng.normal(0.0, 0.01, (10000, 3)))
    there, back = np.eye(4), np.eye(4)
    there[:3, 3], back[:3, 3] = at, -at
    T0 = np.ascontiguousarray(there @ rigid(0.01, -0.02, np.deg2rad(2.0), [1.0, 0.1, 0.0]) @ back)
    T0[3] = (0.0, 0.0, 0.0, 1.0)
    params = mod.kitti_params(max_num_iterations=6, max_num_se3_iterations=3)
    edges, init = [(0, 1), (1, 0)], [T0, None]  # A posed, then A itself as a target
    runs = {}
    try:
        for mode in (0, 1):
            mod.set_pose_seeding(mode)
            res = mod.register_graph([A, B], edges, "se3_gicp", params, sharing=2, init=init)
            runs[mode] = ([_bytes(r) for r in res], mod.last_init_stats(), mod.last_seed_stats())
    finally:
        mod.set_pose_seeding(0)
    print(f"[init] utm seeding: on {runs[0][1]} {runs[0][2]}; off {runs[1][1]} {runs[1][2]}")
    parity_record("init: utm seeding", **runs[0][1], **runs[0][2])
    assert runs[0][0] == runs[1][0]
    assert runs[0][1]["classes_seeded_across"] >= 1 and runs[1][1]["classes_seeded_across"] == 0


# ------------------------------------------------------------------ 7. confidence-weighted GICP
def test_cf_z_preserving_pose(se3icp_mod, bunny_clouds, parity_record):
    """Rotation about z and a translation in xy, the third row exactly (0, 0, 1, 0): z is bitwise
    unchanged, so the raw confidences are X''s and the plain entry on X' is matched."""
    c, s = np.cos(0.03), np.sin(0.03)
    T0 = np.array([[c, -s, 0.0, 0.004], [s, c, 0.0, -0.003], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    X = bunny_clouds[0]
    assert np_apply(T0, X)[:, 2].tobytes() == X[:, 2].tobytes()
    check_posed(se3icp_mod, parity_record, "B cf z-preserving", bunny_clouds, [(0, 1), (2, 1)], [T0, None],
                "se3_gicp_with_cf", se3icp_mod.default_params())


def test_cf_tilted_pose_takes_raw_confidences(se3icp_mod, bunny_unique, parity_record):
    """The stated departure: under a pose that tilts the cloud the source's confidences are the RAW
    depths'.  The pose is a quarter turn about x, (x, y, z) -> (x, -z, y): it keeps exact_cf_pair's
    grid and symmetry, so the normalization of (X', target) is exact, the trace is in the
    inputs' frame and its first step can be recomputed in long double with either weighting."""
    from test_gpu_steps import (CF_PARAMS, POSE_CONDITION, _normals_for, exact_cf_pair, jacobian_step_deviation,
                                lounge_confidence)
    mod = se3icp_mod
    src, tgt = exact_cf_pair(bunny_unique, 129)
    T0 = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    moved = np_apply(T0, src)
    assert not moved.sum(0).any() and np.array_equal(moved[:, 1], -src[:, 2]) and np.array_equal(moved[:, 2], src[:, 1])
    gp = mod.default_params(**CF_PARAMS)
    res, tr = mod.register_graph_traced([np.array(src), np.array(tgt)], [(0, 1)], "se3_gicp_with_cf", gp, edge=0,
                                        max_iters=10, init=[T0])
    assert res[0].status == 0 and res[0].scaling_factor == 1.0 and len(tr["T"]) >= 1
    nt, ns0 = _normals_for("cf", mod, (moved, tgt))
    conf_t = lounge_confidence(tgt[:, 2])
    dev = {}
    for name, z in (("raw", src[:, 2]), ("moved", moved[:, 2])):
        dev[name] = jacobian_step_deviation("cf", moved, tgt, tr["corr_idx"], tr["corr_dist"], tr["T"], tr["mse"],
                                            CF_PARAMS["estimated_overlap"], nt, ns0, (lounge_confidence(z), conf_t),
                                            its=[0])
    bar = POSE_CONDITION * max(dev["raw"][2], dev["moved"][2])
    print(f"[init] cf tilted: |T - T_ld|_F raw weights {dev['raw'][0]:.2e}, moved weights {dev['moved'][0]:.2e}, bar {bar:.2e}")
    parity_record("init: cf tilted first step", raw_dev=dev["raw"][0], moved_dev=dev["moved"][0], bar=bar)
    assert dev["raw"][0] <= bar, dev
    assert dev["moved"][0] > bar, dev


# ------------------------------------------------------------------ 8. that it is good for something
FAR_DEG = 120.0  # picked with oracle/refcpu on the CPU: see test_init_host.py::test_oracle_misses_without_a_pose


def _rz(deg):
    return rigid(0.0, 0.0, np.deg2rad(deg), [0.0, 0.0, 0.0])


def test_far_start_needs_the_pose(se3icp_mod, fixture_clouds, fixture_T_gt):
    mod = se3icp_mod
    src, tgt = fixture_clouds
    Z = _rz(FAR_DEG)
    far = np.ascontiguousarray(src @ Z[:3, :3].T)
    lost = mod.register_graph([far, tgt], [(0, 1)], "se3_pt2pl")[0]
    miss = np.linalg.norm(lost.T @ Z - fixture_T_gt)
    guess = rigid(np.deg2rad(3.0), np.deg2rad(-3.0), np.deg2rad(-FAR_DEG + 2.6), [0.0, 0.0, 0.0])
    got = mod.register_graph([far, tgt], [(0, 1)], "se3_pt2pl", init=[guess])[0]
    err = np.linalg.norm(got.T @ Z - fixture_T_gt)
    print(f"[init] far start {FAR_DEG} deg: without a pose {miss:.3e} from the truth, with one {err:.3e}")
    assert miss > 0.1
    assert got.status == 0 and err <= 1e-6, err


LOOP_DEG = 150.0


def loop_closure_problem(scans, poses, mod):
    """A two-scan loop closure made from S: scan 4 as a vehicle on its way back records it, the
    sensor turned by LOOP_DEG about z, against scan 0.  Returns (clouds, the absolute poses
    world_T_cloud, the true pose of edge (1, 0))."""
    Z = _rz(LOOP_DEG)
    back = np.ascontiguousarray(scans[4] @ Z[:3, :3].T)
    P = [poses[0], poses[4] @ np.linalg.inv(Z)]
    return [scans[0], back], P, np.linalg.inv(P[0]) @ P[1]


def test_loop_closure_through_edge_inits(se3icp_mod, parity_record):
    """Without a pose the edge ends far from the truth (the oracle too:
    test_init_host.py::test_oracle_misses_the_loop_closure); with the relative pose of drifted
    absolute poses (a degree of yaw, a third of a metre) it ends within 1 cm of it -- the scans
    carry 2 cm of range noise, and the oracle from the same start ends 2.4 mm from it."""
    from se3icp import datasets
    mod = se3icp_mod
    sc, poses = datasets.kitti_like_sequence(5, seed=4, n_az=200)
    clouds, P, truth = loop_closure_problem([np.ascontiguousarray(x, dtype=np.float64) for x in sc], poses, mod)
    drift = rigid(0.0, 0.0, np.deg2rad(1.0), [0.3, -0.2, 0.0])
    init = mod.edge_inits([P[0], drift @ P[1]], [(1, 0)])
    lost = mod.register_graph(clouds, [(1, 0)], "se3_gicp", mod.kitti_params())[0]
    got = mod.register_graph(clouds, [(1, 0)], "se3_gicp", mod.kitti_params(), init=init)[0]
    miss, err, guess = (np.linalg.norm(M - truth) for M in (lost.T, got.T, init[0]))
    print(f"[init] loop closure: guess {guess:.3f} off, without a pose {miss:.3f}, with it {err:.2e}")
    parity_record("init: loop closure", guess_off=guess, without_pose=miss, with_pose=err)
    assert miss > 1.0
    assert got.status == 0 and err <= 0.01 < guess


# ------------------------------------------------------------------ 9. unchanged calls
@pytest.mark.parametrize("method", ["se3_gicp", "gicp"])
def test_unposed_calls_are_the_plain_graph(se3icp_mod, scans, method):
    mod = se3icp_mod
    edges = mod.sequence_edges(5)
    params = mod.kitti_params()
    want = [_bytes(r) for r in mod.register_graph(scans, edges, method, params)]
    stats = mod.last_graph_stats()
    for init in (None, [None] * 4, [np.eye(4)] * 4):
        assert [_bytes(r) for r in mod.register_graph(scans, edges, method, params, init=init)] == want
    # the C entry itself with an all-identity table, and with NULL
    import ctypes as C
    from se3icp import _lib
    from se3icp.registration import _cloud_args, _edge_arrays, _outputs, _params_ref
    _keep, cargs = _cloud_args(scans)
    n, es, et = _edge_arrays(edges)
    ident = np.ascontiguousarray(np.stack([np.eye(4)] * n))
    for T in (ident.ctypes.data_as(C.POINTER(C.c_double)), None):
        res, _ = _outputs(n)
        rc = _lib.load().se3icp_register_graph_init(0, *cargs, n, es, et, T, _lib.method_id(method), _params_ref(params), 0,
                                                    res, None, None)
        assert rc == 0
        assert [(np.array(r.T).reshape(4, 4).tobytes(), r.num_iterations, r.num_pure_se3_iterations, r.status,
                 np.float64(r.scaling_factor).tobytes()) for r in res[:n]] == want
        assert mod.last_init_stats() == {"posed_edges": 0, "posed_variants": 0, "classes_seeded_across": 0}
        assert mod.last_graph_stats() == stats
