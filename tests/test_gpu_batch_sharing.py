"""GPU tests of content-detected sharing in the device batch entries
(se3icp_register_batch_device, se3icp_register_batch_report_device; se3icp_set_batch_sharing).

A device batch is 2P cloud slots; a chain of scans expanded into pairs holds every interior
scan twice.  The entries hash every slot's raw bytes on the device, confirm equal hashes with a
byte-for-byte compare and then select neighbours once per (cloud, normalization) class, on the
slots as they lie.  The bar needs no oracle and no tolerance: results[p] is bitwise what the
same call returns with sharing off (level 1) -- T, both iteration counts, status and
scaling_factor -- and se3icp_last_graph_stats says what was shared.

Neighbour-set adoption between the classes of one cloud is not built: the four adoption
counters stay 0, which the tests assert.

Inputs:
  S     datasets.kitti_like_sequence(5, seed=4, n_az=200), ~12.5k points a scan, as
        tests/test_gpu_graph.py: under the run_se3_* normalization scan 1 is one class for both
        of its uses, scans 2 and 3 are two classes each
  B     clouds cut from the bunny (a few thousand points and less, odd sizes)
Every use is a copy of its own in the device buffers: nothing is shared by address.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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
    """Four different clouds of 3,001 .. 3,544 points (rigidly moved, noisy bunny subsets)."""
    from se3icp import datasets
    out = []
    for seed in (2, 3):
        src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=seed, subsample=0.1)
        out += [src, tgt]
    out[2] = out[2][:3001].copy()
    return [np.ascontiguousarray(c, dtype=np.float64) for c in out]


def _bytes(r):
    return (r.T.tobytes(), r.num_iterations, r.num_pure_se3_iterations, r.status, np.float64(r.scaling_factor).tobytes())


class DeviceBatch:
    """The pairs' clouds in two device buffers (sources, targets), every use a copy of its own."""

    def __init__(self, pairs, stream=None):
        import torch
        self.src_off = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
        self.tgt_off = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
        src = np.ascontiguousarray(np.concatenate([s for s, _ in pairs]), dtype=np.float64)
        tgt = np.ascontiguousarray(np.concatenate([t for _, t in pairs]), dtype=np.float64)
        if stream is None:
            self.d_src, self.d_tgt = torch.from_numpy(src).to("cuda"), torch.from_numpy(tgt).to("cuda")
            torch.cuda.synchronize()
        else:
            with torch.cuda.stream(stream):
                self.d_src, self.d_tgt = torch.from_numpy(src).to("cuda"), torch.from_numpy(tgt).to("cuda")
            stream.synchronize()
        # (bytes, not values: a -0.0 or a NaN payload must arrive as it was written)
        assert self.d_src.cpu().numpy().tobytes() == src.tobytes()

    def args(self):
        return self.d_src.data_ptr(), self.src_off, self.d_tgt.data_ptr(), self.tgt_off


def _run(mod, batch, method, params, level, device=0, stream=0):
    """One device batch at sharing `level`; returns (results, graph stats -- None at level 1, which
    does not write them)."""
    mod.set_batch_sharing(level, device)
    try:
        res = mod.register_batch_device(*batch.args(), method, params, device=device, stream=stream)
        return res, (mod.last_graph_stats(device) if level != 1 else None)
    finally:
        mod.set_batch_sharing(0, device)


def _parity(mod, parity_record, name, pairs, method, params, device=0):
    """Default level and level 2 against level 1, bitwise; returns (plain results, default stats)."""
    batch = DeviceBatch(pairs)
    want, _ = _run(mod, batch, method, params, 1, device)
    out = None
    for level in (0, 2):
        got, st = _run(mod, batch, method, params, level, device)
        bad = [p for p in range(len(pairs)) if _bytes(got[p]) != _bytes(want[p])]
        print(f"[batch sharing] {name} level {level}: {len(pairs)} pairs, {len(bad)} differ; {st}")
        parity_record(f"batch sharing: {name} level {level}", pairs=len(pairs), differ=len(bad), **st)
        assert not bad, [(p, got[p], want[p]) for p in bad[:2]]
        assert st["uses"] == 2 * len(pairs)
        assert st["adopted"] == st["rejected_order"] == st["rejected_gap"] == st["no_list"] == 0
        assert st["bytes_uploaded"] == 0
        out = out or st
        assert st == out  # level 0 is level 2
    return want, out


# ------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("method", ["se3_gicp", "se3_pt2pl", "se3_gicp_with_cf", "gicp"])
def test_chain_parity(se3icp_mod, scans, parity_record, method):
    """Scan i+1 onto scan i over five scans: eight slots, five clouds."""
    pairs = se3icp_mod.expand_edges(scans, se3icp_mod.sequence_edges(5))
    want, st = _parity(se3icp_mod, parity_record, f"S {method}", pairs, method, se3icp_mod.kitti_params())
    assert all(r.status == 0 for r in want) and len({_bytes(r) for r in want}) == 4
    assert (st["clouds"], st["uses"]) == (5, 8), st
    if method.startswith("se3"):
        # scan 1: the scale of both its pairs is 3 / r_1; scans 2 and 3: two scales each
        assert (st["classes"], st["classes_full"]) == (7, 7), st
    else:
        # gicp, raw coordinates: a cloud's classes differ in the f32 centre (the pair's target)
        # only, so each cloud computes its normals once
        assert (st["classes"], st["classes_full"]) == (8, 5), st


def test_chain_selects_once_per_class(se3icp_mod, scans):
    """The kNN / frame kernels select for 7 classes, not 8 slots (lrf_queries counts a handed-over
    query in both kernels that took it)."""
    pairs = se3icp_mod.expand_edges(scans, se3icp_mod.sequence_edges(5))
    batch = DeviceBatch(pairs)
    params = se3icp_mod.kitti_params()
    _run(se3icp_mod, batch, "se3_gicp", params, 1)
    kb = se3icp_mod.last_kernel_times()
    _run(se3icp_mod, batch, "se3_gicp", params, 0)
    k2 = se3icp_mod.last_kernel_times()
    n1 = scans[1].shape[0]
    saved = kb["lrf_queries"] - k2["lrf_queries"]
    assert n1 <= saved <= n1 + kb["lrf_fallback"], (saved, n1, kb["lrf_fallback"])


# ------------------------------------------------------------------ 2. collisions
def _next_up(x):
    return np.nextafter(x, np.inf)


def test_one_ulp_apart_is_not_shared(se3icp_mod, bunny_clouds, parity_record):
    """Equal-length clouds that differ in one coordinate by one ulp, and a pair of clouds that
    differ in the sign of one zero, are two clouds each."""
    a = bunny_clouds[0][:2500].copy()
    b = a.copy()
    b[1234, 1] = _next_up(b[1234, 1])
    z0 = bunny_clouds[1][:2000].copy()
    z0[77, 2] = 0.0
    z1 = z0.copy()
    z1[77, 2] = -0.0
    assert a.tobytes() != b.tobytes() and z0.tobytes() != z1.tobytes() and np.array_equal(z0, z1)
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=5, max_num_iterations=20)
    for name, pairs, clouds in [("ulp", [(a, b)], 2), ("signed zero", [(z0, z1)], 2),
                                ("both", [(a, b), (z1, z0), (b, a)], 4)]:
        _, st = _parity(se3icp_mod, parity_record, f"collision guard {name}", pairs, "se3_gicp", params)
        assert st["clouds"] == clouds, (name, st)
    # the same bytes in two slots are one cloud (a NaN-free control for the cases above)
    _, st = _parity(se3icp_mod, parity_record, "collision guard control", [(a, a.copy())], "se3_gicp", params)
    assert (st["clouds"], st["classes"], st["classes_full"]) == (1, 1, 1), st


# ------------------------------------------------------------------ 3. nothing to share
def test_no_duplicates(se3icp_mod, bunny_clouds, parity_record):
    """Distinct clouds: every slot its own cloud and class, results bitwise level 1's -- with
    equal point counts (hashed, no hash agrees) and without (nothing is hashed)."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=5, max_num_iterations=20)
    c = bunny_clouds
    equal_n = [(c[0][:3000], c[1][:3000]), (c[2][:3000], c[3][:3000])]
    distinct_n = [(c[0][:2999], c[1][:3000]), (c[2][:3001], c[3][:2998])]
    for name, pairs in [("equal n", equal_n), ("distinct n", distinct_n)]:
        for method, full in [("se3_gicp", 4), ("pt2pl", 2)]:
            _, st = _parity(se3icp_mod, parity_record, f"no duplicates {name} {method}", pairs, method, params)
            assert (st["clouds"], st["uses"], st["classes"], st["classes_full"]) == (4, 4, 4, full), st
    # the plain path: as many selected queries as at level 1
    batch = DeviceBatch(equal_n)
    _run(se3icp_mod, batch, "se3_gicp", params, 1)
    k1 = se3icp_mod.last_kernel_times()
    _run(se3icp_mod, batch, "se3_gicp", params, 0)
    k0 = se3icp_mod.last_kernel_times()
    assert (k0["lrf_queries"], k0["lrf_fallback"]) == (k1["lrf_queries"], k1["lrf_fallback"])


# ------------------------------------------------------------------ 4. ties
def _lattice(n, h):
    g = np.arange(n, dtype=np.float64) * h
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_ties_under_two_scales(se3icp_mod, parity_record):
    """Integer lattices (exact distance ties, decided by the hand-over to the exact kernel), one
    of them inside two pairs of different radii."""
    clouds = [_lattice(11, 1.0), _lattice(12, 1.0), _lattice(10, 2.0)]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2), (0, 0)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=12)
    batch = DeviceBatch(pairs)
    _, st = _parity(se3icp_mod, parity_record, "ties", pairs, "se3_gicp", params)
    assert st["clouds"] == 3 and st["classes"] > st["clouds"], st  # some lattice runs under two scales
    assert st["classes"] < st["uses"], st                          # and the self pair is one class
    _run(se3icp_mod, batch, "se3_gicp", params, 0)
    assert se3icp_mod.last_kernel_times()["lrf_fallback"] > 0       # tied queries reach the exact kernel


# ------------------------------------------------------------------ 5. structural sizes
@pytest.mark.parametrize("k", [30, 90, 127, 128, 150])
def test_small_clouds(se3icp_mod, bunny_clouds, parity_record, k):
    """n <= Kw, n = Kw + 1, partial waves only; k at and over what the LDS kernels hold."""
    base = bunny_clouds[0]
    clouds = [np.ascontiguousarray(base[o:o + n] * (1.0 + 0.1 * i))
              for i, (o, n) in enumerate([(0, 7), (10, 8), (20, 9), (40, 64), (100, 65), (200, 90), (300, 91),
                                          (400, 92), (500, 131)])]
    edges = se3icp_mod.sequence_edges(len(clouds)) + [(0, 8), (8, 3)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=k, max_num_se3_iterations=3, max_num_iterations=8)
    _, st = _parity(se3icp_mod, parity_record, f"small k={k}", se3icp_mod.expand_edges(clouds, edges), "se3_gicp", params)
    assert st["clouds"] == 9 and st["classes"] < st["uses"], st


def test_full_tree_nodes(se3icp_mod, bunny_unique, parity_record):
    """4,096 and 4,097 points: a full local tree node and one point over."""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])[:4097]], dtype=np.float64)
    clouds = [pts[:4096].copy(), pts * 1.3 + 0.01, pts[1:4097] * 0.8]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=10)
    _, st = _parity(se3icp_mod, parity_record, "4096/4097", pairs, "se3_gicp", params)
    assert (st["clouds"], st["classes"]) == (3, 5), st  # cloud 1 has the largest radius of both its pairs


# ------------------------------------------------------------------ 6. other paths
CHAIN_B = [(1, 0), (2, 1), (3, 1), (1, 1)]


def test_report_with_per_point_outputs(se3icp_mod, bunny_clouds, parity_record):
    import torch
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60, estimated_overlap=0.7, mse_switch_error=5e-5)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    batch = DeviceBatch(pairs)
    total = int(batch.src_off[-1])
    out = {}
    for level in (1, 0):
        idx = torch.full((total,), -1, dtype=torch.int32, device="cuda")
        dist = torch.zeros(total, dtype=torch.float64, device="cuda")
        se3icp_mod.set_batch_sharing(level)
        try:
            res, rep = se3icp_mod.register_batch_report_device(*batch.args(), "se3_gicp", params,
                                                               max_correspondence_distance=0.02,
                                                               corr_idx_ptr=idx.data_ptr(), corr_dist_ptr=dist.data_ptr())
        finally:
            se3icp_mod.set_batch_sharing(0)
        torch.cuda.synchronize()
        out[level] = (res, rep, idx.cpu().numpy(), dist.cpu().numpy())
    st = se3icp_mod.last_graph_stats()
    assert st["clouds"] == 4 and st["classes"] < st["uses"], st
    (r1, p1, i1, d1), (r0, p0, i0, d0) = out[1], out[0]
    assert [_bytes(r) for r in r0] == [_bytes(r) for r in r1]
    for a, b in zip(p0, p1):
        assert (a.fitness, a.inlier_rmse, a.final_mse, a.final_mse_change, a.n_inliers, a.switched, a.stop_reason) == \
               (b.fitness, b.inlier_rmse, b.final_mse, b.final_mse_change, b.n_inliers, b.switched, b.stop_reason)
        assert np.array_equal(a.information, b.information)
    assert (i0 >= 0).all() and np.array_equal(i0, i1) and d0.tobytes() == d1.tobytes()
    parity_record("batch sharing: report", pairs=len(pairs), points=total)


def test_trace_on_a_sharing_use(se3icp_mod, scans, parity_record):
    """Every row of the search to the bit: the per-iteration record of pair 1 of the chain, whose
    target takes its frames from pair 0's source."""
    from se3icp import registration
    pairs = se3icp_mod.expand_edges(scans, se3icp_mod.sequence_edges(5))
    batch = DeviceBatch(pairs)
    params = se3icp_mod.kitti_params()
    rec = {}
    for level in (1, 0):
        se3icp_mod.set_batch_sharing(level)
        try:
            with registration._armed_trace(0, 1, pairs[1][0].shape[0], 160) as tr:
                res = se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params)
        finally:
            se3icp_mod.set_batch_sharing(0)
        rec[level] = (res, tr)
    assert rec[1][1]["phase"].shape[0] > 2
    for key in ("corr_idx", "corr_dist", "trim_key", "T", "mse", "phase"):
        assert rec[0][1][key].shape == rec[1][1][key].shape, key
        assert np.array_equal(rec[0][1][key], rec[1][1][key]), key
    assert [_bytes(r) for r in rec[0][0]] == [_bytes(r) for r in rec[1][0]]
    parity_record("batch sharing: trace pair 1", iterations=int(rec[0][1]["phase"].shape[0]))


def test_engine_slot_and_callers_stream(se3icp_mod, bunny_clouds, parity_record):
    """A further engine of the same GPU (device | slot << 8) whose first call shares, and a call
    on the caller's stream."""
    import torch
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    want, st0 = _parity(se3icp_mod, parity_record, "slot 0", pairs, "se3_gicp", params)
    got, st1 = _parity(se3icp_mod, parity_record, "slot 1", pairs, "se3_gicp", params, device=0 | 1 << 8)
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want] and st0 == st1
    stream = torch.cuda.Stream()
    batch = DeviceBatch(pairs, stream)
    res, st = _run(se3icp_mod, batch, "se3_gicp", params, 0, stream=stream.cuda_stream)
    stream.synchronize()
    assert [_bytes(r) for r in res] == [_bytes(r) for r in want] and st == st0


@pytest.mark.parametrize("mode", [1, 2])
def test_lrf_exact_modes(se3icp_mod, bunny_clouds, parity_record, mode):
    """se3icp_set_lrf_exact: every class through the selected exact kernel."""
    from se3icp import registration
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    want, _ = _run(se3icp_mod, DeviceBatch(pairs), "se3_gicp", params, 1)
    registration.set_lrf_exact(mode)
    try:
        got, _ = _parity(se3icp_mod, parity_record, f"lrf_exact {mode}", pairs, "se3_gicp", params)
    finally:
        registration.set_lrf_exact(0)
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want]


def test_then_a_plain_host_batch(se3icp_mod, bunny_clouds):
    """A host batch right after a shared call returns what it returned before it, and the host
    entry itself does not look: it selects for every use."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    b0 = se3icp_mod.register_batch(pairs, "se3_gicp", params)
    k0 = se3icp_mod.last_kernel_times()
    _, st = _run(se3icp_mod, DeviceBatch(pairs), "se3_gicp", params, 0)
    ks = se3icp_mod.last_kernel_times()
    assert st["classes_full"] < st["uses"] and ks["lrf_queries"] < k0["lrf_queries"]
    b1 = se3icp_mod.register_batch(pairs, "se3_gicp", params)
    k1 = se3icp_mod.last_kernel_times()
    assert [_bytes(r) for r in b0] == [_bytes(r) for r in b1]
    assert (k1["lrf_queries"], k1["lrf_fallback"]) == (k0["lrf_queries"], k0["lrf_fallback"])
