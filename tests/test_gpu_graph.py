"""GPU tests of registration over a shared cloud set (se3icp_register_graph): every distinct
cloud uploaded and ingested once, the neighbours, frames and normals of every (cloud,
normalization) class selected once, every result bitwise what register_batch returns for the
expanded pair list.

The bar needs no oracle and no tolerance: a pair registers bit for bit the same alone or in
any batch, a use is normalized with k_normalize's arithmetic from the shared raw columns, and
k_graph_share hands a class's rows to its other uses through the frame kernels' epilogue.  So
every comparison is on the bytes of T plus num_iterations, num_pure_se3_iterations, status and
scaling_factor against register_batch on the same build, at sharing 1, 2 and 3.

Neighbour-set adoption between the classes of one cloud (sharing 3 of the interface) is not
built: level 3 runs as level 2 and the adoption counters stay 0, which the tests assert.

Inputs:
  S     datasets.kitti_like_sequence(5, seed=4, n_az=200): ~12.5k points a scan, radii
        69.15, 74.58, 73.83, 69.71, 71.00 -- under the run_se3_* normalization scan 1 is one
        class for both of its uses, scans 2 and 3 are two classes each
  B     clouds cut from the bunny (a few thousand points and less, odd sizes)
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
    s = [np.ascontiguousarray(x, dtype=np.float64) for x in s]
    rad = [float(np.sqrt(((x - x.mean(0)) ** 2).sum(1)).max()) for x in s]
    # what the class structure below rests on: scan 1 has the largest radius of its two pairs
    assert rad[1] > rad[0] and rad[1] > rad[2] and rad[2] > rad[3] and rad[4] > rad[3], rad
    return s


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


def _check(mod, parity_record, name, clouds, edges, method, params, levels=LEVELS, device=0, want=None):
    """The graph call at every sharing level against register_batch on the expanded pairs;
    returns (batch results, {level: stats})."""
    if want is None:
        want = mod.register_batch(mod.expand_edges(clouds, edges), method, params)
    stats = {}
    for lv in levels:
        got = mod.register_graph(clouds, edges, method, params, device=device, sharing=lv)
        stats[lv] = mod.last_graph_stats(device)
        assert len(got) == len(edges)
        bad = [p for p in range(len(edges)) if _bytes(got[p]) != _bytes(want[p])]
        print(f"[graph] {name} sharing {lv}: {len(edges)} edges, {len(bad)} differ; {stats[lv]}")
        parity_record(f"graph: {name} sharing {lv}", edges=len(edges), differ=len(bad), **stats[lv])
        assert not bad, [(p, got[p], want[p]) for p in bad[:2]]
        st = stats[lv]
        assert st["uses"] == 2 * len(edges)
        assert st["clouds"] == len({c for e in edges for c in e})
        assert st["adopted"] == st["rejected_order"] == st["rejected_gap"] == st["no_list"] == 0
        assert st["bytes_uploaded"] == 24 * sum(clouds[c].shape[0] for c in {c for e in edges for c in e})
        if lv == 1:
            assert st["classes"] == st["classes_full"] or method in ("pt2pt", "pt2pl", "gicp")
            assert st["classes"] == 2 * len(edges)
    return want, stats


# ------------------------------------------------------------------ 1. the sequence
SEQ_METHODS = ["se3_gicp", "se3_pt2pt", "se3_pt2pl", "se3_gicp_with_cf", "se3_pure_gicp", "gicp", "pt2pt"]


@pytest.mark.parametrize("method", SEQ_METHODS)
def test_sequence(se3icp_mod, scans, parity_record, method):
    """Scan i+1 onto scan i over five scans: eight uses of five clouds."""
    edges = se3icp_mod.sequence_edges(5)
    assert edges == [(1, 0), (2, 1), (3, 2), (4, 3)]
    params = se3icp_mod.kitti_params()
    want, stats = _check(se3icp_mod, parity_record, f"S {method}", scans, edges, method, params)
    assert all(r.status == 0 for r in want)
    assert len({_bytes(r) for r in want}) == 4
    for lv in (2, 3):
        st = stats[lv]
        if method.startswith("se3"):
            # scan 1: the scale of both its pairs is 3 / r_1; scans 2 and 3: two scales each
            assert (st["classes"], st["classes_full"]) == (7, 7), st
        elif method == "gicp":
            # raw coordinates: a cloud's classes differ in the f32 centre (the pair's target)
            # only, so each cloud computes its normals once
            assert (st["classes"], st["classes_full"]) == (8, 5), st
        else:
            assert (st["classes"], st["classes_full"]) == (8, 0), st  # pt2pt: no kNN at all
    # the register_sequence spelling
    got = se3icp_mod.register_sequence(scans, method, params)
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want]


def test_sequence_setup_is_shared(se3icp_mod, scans, parity_record):
    """The kNN / frame kernels select for 7 classes, not 8 uses; sharing 1 selects for all 8.
    (lrf_queries counts a handed-over query in both kernels that took it.)"""
    edges = se3icp_mod.sequence_edges(5)
    params = se3icp_mod.kitti_params()
    n = [s.shape[0] for s in scans]
    se3icp_mod.register_batch(se3icp_mod.expand_edges(scans, edges), "se3_gicp", params)
    kb = se3icp_mod.last_kernel_times()
    assert kb["lrf_queries"] >= n[0] + 2 * (n[1] + n[2] + n[3]) + n[4]
    se3icp_mod.register_graph(scans, edges, "se3_gicp", params, sharing=1)
    k1 = se3icp_mod.last_kernel_times()
    assert (k1["lrf_queries"], k1["lrf_fallback"]) == (kb["lrf_queries"], kb["lrf_fallback"])
    se3icp_mod.register_graph(scans, edges, "se3_gicp", params, sharing=2)
    k2 = se3icp_mod.last_kernel_times()
    saved = kb["lrf_queries"] - k2["lrf_queries"]
    assert n[1] <= saved <= n[1] + kb["lrf_fallback"], (saved, n[1], kb["lrf_fallback"])
    parity_record("graph: S shared setup", lrf_queries_graph=k2["lrf_queries"], lrf_queries_batch=kb["lrf_queries"],
                  lrf_fallback_batch=kb["lrf_fallback"], points_scan_1=n[1])


# ------------------------------------------------------------------ 2. one map, many scans
@pytest.mark.parametrize("method", ["se3_gicp", "gicp", "pt2pl"])
def test_one_map(se3icp_mod, scans, parity_record, method):
    """Scan 1 is the target of scans 0, 2 and 3, of itself, and of scan 0 once more."""
    edges = [(0, 1), (2, 1), (3, 1), (1, 1), (0, 1)]
    params = se3icp_mod.kitti_params()
    want, stats = _check(se3icp_mod, parity_record, f"map {method}", scans, edges, method, params)
    assert _bytes(want[0]) == _bytes(want[4])
    st = stats[2]
    # scan 1 has the largest radius of every pair: one scale, and one f32 centre (its own)
    # for the vanilla methods -- one target class; sources 0, 2, 3
    assert st["classes"] == 4 and st["clouds"] == 4, st
    assert st["classes_full"] == {"se3_gicp": 4, "gicp": 4, "pt2pl": 1}[method], st


def test_edge_order_and_unused_cloud(se3icp_mod, scans, parity_record):
    """Edges in any order over a cloud list with an unused (and an empty unused) cloud."""
    clouds = [scans[3], np.zeros((0, 3)), scans[0], scans[4], scans[1]]
    edges = [(4, 2), (0, 4), (2, 0)]
    _, stats = _check(se3icp_mod, parity_record, "order", clouds, edges, "se3_gicp", se3icp_mod.kitti_params())
    assert stats[2]["clouds"] == 3


# ------------------------------------------------------------------ 3. ties
def _mirrored(rng, n_pairs, spread):
    q = rng.uniform(-spread, spread, (n_pairs, 3))
    v = rng.uniform(-0.05, 0.05, (n_pairs, 3)) * spread
    return np.ascontiguousarray(np.concatenate([q + v, q - v, q[: n_pairs // 3]]))


def _lattice(n, h):
    g = np.arange(n, dtype=np.float64) * h
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_ties(se3icp_mod, parity_record):
    """Exact distance ties (mirrored point pairs about shared centres, lattices) under two
    scales: the hand-over to the exact kernel decides them, the same in a graph and a batch."""
    rng = np.random.default_rng(7)
    clouds = [_mirrored(rng, 600, 1.0), _mirrored(rng, 700, 1.5), _mirrored(rng, 500, 2.0),
              _lattice(11, 0.25), _lattice(12, 0.3), _lattice(10, 0.5)]
    edges = [(1, 0), (2, 1), (0, 2), (4, 3), (5, 4), (3, 5)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=12)
    _, stats = _check(se3icp_mod, parity_record, "ties", clouds, edges, "se3_gicp", params)
    assert stats[2]["classes"] > stats[2]["clouds"]  # some cloud runs under two scales


# ------------------------------------------------------------------ 4. structural sizes
@pytest.mark.parametrize("k", [30, 90, 127, 128, 150])
def test_small_clouds(se3icp_mod, bunny_clouds, parity_record, k):
    """n <= Kw, n = Kw + 1, partial waves only; k at and over what the LDS kernels hold."""
    base = bunny_clouds[0]
    clouds = [np.ascontiguousarray(base[o:o + n] * (1.0 + 0.1 * i))
              for i, (o, n) in enumerate([(0, 7), (10, 8), (20, 9), (40, 64), (100, 65), (200, 90), (300, 91),
                                          (400, 92), (500, 131)])]
    edges = se3icp_mod.sequence_edges(len(clouds)) + [(0, 8), (8, 3)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=k, max_num_se3_iterations=3, max_num_iterations=8)
    _check(se3icp_mod, parity_record, f"small k={k}", clouds, edges, "se3_gicp", params)


def test_full_tree_nodes(se3icp_mod, bunny_unique, parity_record):
    """4,096 and 4,097 points: a full local tree node and one point over."""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])[:4097]], dtype=np.float64)
    clouds = [pts[:4096].copy(), pts * 1.3 + 0.01, pts[1:4097] * 0.8]
    edges = [(1, 0), (2, 1), (0, 2)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=10)
    _, stats = _check(se3icp_mod, parity_record, "4096/4097", clouds, edges, "se3_gicp", params)
    assert stats[2]["classes"] == 5, stats[2]  # cloud 1 has the largest radius of both its pairs


def test_normals_k_over_frames_k(se3icp_mod, bunny_clouds, parity_record):
    """se3_pt2pl with number_of_nn_for_LRF = 10: a class that is a source (no normals, 10
    neighbours) and a target (30) selects 30 for both; the frames take the first 10."""
    edges = [(1, 0), (2, 1), (3, 1), (0, 1)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=10, max_num_se3_iterations=5, max_num_iterations=20)
    _check(se3icp_mod, parity_record, "B se3_pt2pl k=10", bunny_clouds, edges, "se3_pt2pl", params)


# ------------------------------------------------------------------ 5. other paths
def test_trace_on_shared_class(se3icp_mod, scans, parity_record):
    """Every row of the SE(3) search to the bit: the per-iteration record of edge (2, 1), whose
    target is the class both uses of scan 1 share and whose source is scan 2's second class."""
    edges = se3icp_mod.sequence_edges(5)
    params = se3icp_mod.kitti_params()
    res, tr = se3icp_mod.register_graph_traced(scans, edges, "se3_gicp", params, edge=1)
    ref_res, ref_tr = se3icp_mod.register_batch_traced(se3icp_mod.expand_edges(scans, edges), "se3_gicp", params, pair=1)
    assert ref_tr["phase"].shape[0] > 2
    for key in ("corr_idx", "corr_dist", "trim_key", "T", "mse", "phase"):
        assert tr[key].shape == ref_tr[key].shape, key
        assert np.array_equal(tr[key], ref_tr[key]), key
    assert [_bytes(r) for r in res] == [_bytes(r) for r in ref_res]
    parity_record("graph: trace edge 1", iterations=int(tr["phase"].shape[0]), correspondences=int(tr["corr_idx"].size))
    # the trace disarmed itself
    again = se3icp_mod.register_graph(scans, edges, "se3_gicp", params)
    assert [_bytes(r) for r in again] == [_bytes(r) for r in ref_res]


def test_report(se3icp_mod, bunny_clouds, parity_record):
    edges = [(1, 0), (2, 1), (3, 1), (1, 1)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60, estimated_overlap=0.7, mse_switch_error=5e-5)
    pairs = se3icp_mod.expand_edges(bunny_clouds, edges)
    want, wrep = se3icp_mod.register_batch_report(pairs, "se3_gicp", params, max_correspondence_distance=0.02,
                                                  per_point=True)
    got, grep = se3icp_mod.register_graph_report(bunny_clouds, edges, "se3_gicp", params,
                                                 max_correspondence_distance=0.02, per_point=True)
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want]
    for a, b in zip(grep, wrep):
        assert (a.fitness, a.inlier_rmse, a.final_mse, a.final_mse_change, a.n_inliers, a.switched, a.stop_reason) == \
               (b.fitness, b.inlier_rmse, b.final_mse, b.final_mse_change, b.n_inliers, b.switched, b.stop_reason)
        assert np.array_equal(a.information, b.information)
        assert np.array_equal(a.corr_idx, b.corr_idx) and np.array_equal(a.corr_dist, b.corr_dist)
    parity_record("graph: report", edges=len(edges), points=int(sum(r.corr_idx.size for r in grep)))


def test_device_entry(se3icp_mod, bunny_clouds, parity_record):
    import torch
    edges = [(1, 0), (2, 1), (3, 1)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    want = se3icp_mod.register_batch(se3icp_mod.expand_edges(bunny_clouds, edges), "se3_gicp", params)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d = torch.from_numpy(np.concatenate(bunny_clouds)).to("cuda", non_blocking=False)
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in bunny_clouds])])
    for lv in LEVELS:
        got = se3icp_mod.register_graph_device(d.data_ptr(), off, edges, "se3_gicp", params, stream=st.cuda_stream,
                                               sharing=lv)
        st.synchronize()
        assert [_bytes(r) for r in got] == [_bytes(r) for r in want]
        assert se3icp_mod.last_graph_stats()["bytes_uploaded"] == 0
    parity_record("graph: device entry", compared=3 * len(edges))


def test_engine_slot(se3icp_mod, bunny_clouds, parity_record):
    """A further engine of the same GPU (device | slot << 8), whose first call is a graph."""
    edges = [(1, 0), (2, 1), (3, 1)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    want = se3icp_mod.register_batch(se3icp_mod.expand_edges(bunny_clouds, edges), "se3_gicp", params)
    _check(se3icp_mod, parity_record, "engine slot 1", bunny_clouds, edges, "se3_gicp", params, device=0 | 1 << 8,
           want=want)


@pytest.mark.parametrize("mode", [1, 2])
def test_lrf_exact_modes(se3icp_mod, bunny_clouds, parity_record, mode):
    """se3icp_set_lrf_exact: every class through the selected exact kernel."""
    from se3icp import registration
    edges = [(1, 0), (2, 1), (3, 1)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    want = se3icp_mod.register_batch(se3icp_mod.expand_edges(bunny_clouds, edges), "se3_gicp", params)
    registration.set_lrf_exact(mode)
    try:
        _check(se3icp_mod, parity_record, f"lrf_exact {mode}", bunny_clouds, edges, "se3_gicp", params, want=want)
    finally:
        registration.set_lrf_exact(0)


def test_then_a_plain_batch_and_a_sweep(se3icp_mod, bunny_clouds):
    """The graph call swaps engine buffers between its layouts: the plain entries after it
    return what they returned before it."""
    pairs = [(bunny_clouds[0], bunny_clouds[1]), (bunny_clouds[2], bunny_clouds[3])]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    variants = se3icp_mod.sweep_params(params, alpha_rot=[0.3, 3.0])
    b0 = se3icp_mod.register_batch(pairs, "se3_gicp", params)
    s0 = se3icp_mod.register_sweep(pairs, "se3_gicp", variants)
    se3icp_mod.register_graph(bunny_clouds, [(1, 0), (2, 1), (3, 2)], "se3_gicp", params)
    b1 = se3icp_mod.register_batch(pairs, "se3_gicp", params)
    s1 = se3icp_mod.register_sweep(pairs, "se3_gicp", variants)
    assert [_bytes(r) for r in b0] == [_bytes(r) for r in b1]
    assert [[_bytes(r) for r in row] for row in s0] == [[_bytes(r) for r in row] for row in s1]


def test_interleaved_entries_on_one_engine(se3icp_mod, bunny_clouds):
    """The registration entries and the stage entries share one engine's geometry members and
    buffers: a fixed sequence of all of them on engine slot 0 returns, call for call, what the
    same call returns on an engine slot of its own."""
    mod = se3icp_mod
    pairs = [(bunny_clouds[0], bunny_clouds[1]), (bunny_clouds[2], bunny_clouds[3])]
    params = mod.default_params(number_of_nn_for_LRF=60)
    variants = mod.sweep_params(params, alpha_rot=[0.3, 3.0])
    edges = [(1, 0), (2, 1), (3, 2)]
    rng = np.random.default_rng(11)
    q12, d12 = rng.standard_normal((200, 12)), rng.standard_normal((300, 12))
    pts = bunny_clouds[0][:500]
    calls = [
        ("register_batch", lambda d: mod.register_batch(pairs, "se3_gicp", params, device=d)),
        ("nearest_neighbors", lambda d: mod.nearest_neighbors(q12, d12, device=d)),
        ("register_graph", lambda d: mod.register_graph(bunny_clouds, edges, "se3_gicp", params, device=d)),
        ("knn_self", lambda d: mod.knn_self(pts, 8, device=d)),
        ("register_sweep", lambda d: mod.register_sweep(pairs, "se3_gicp", variants, device=d)),
        ("toldi_frames", lambda d: mod.toldi_frames(pts, 30, device=d)),
        ("register_batch_report", lambda d: mod.register_batch_report(pairs, "se3_gicp", params, device=d,
                                                                      max_correspondence_distance=0.05, per_point=True)),
        ("estimate_normals", lambda d: mod.estimate_normals(pts, device=d)),
        ("register_batch", lambda d: mod.register_batch(pairs, "se3_gicp", params, device=d)),
    ]

    def flat(x):  # every value a call returns, as comparable bytes
        if isinstance(x, (list, tuple)):
            return [flat(y) for y in x]
        if isinstance(x, mod.PairResult):
            return _bytes(x)
        if isinstance(x, mod.PairReport):
            f64 = np.array([x.fitness, x.inlier_rmse, x.final_mse, x.final_mse_change])
            return (f64.tobytes(), x.information.tobytes(), x.n_inliers, x.switched, x.stop_reason,
                    x.corr_idx.tobytes(), x.corr_dist.tobytes())
        return (x.dtype.str, x.shape, x.tobytes()) if isinstance(x, np.ndarray) else x

    together = [flat(f(0)) for _, f in calls]
    for k, (name, f) in enumerate(calls):
        alone = flat(f((k + 1) << 8))
        assert together[k] == alone, f"call {k} ({name}) differs from its own-slot twin"
    assert together[0] == together[-1]  # (the same batch before and after everything else)
