"""GPU tests of taking a cloud's first class's neighbour lists in its later classes
(se3icp_set_lrf_taking, se3icp_last_take_stats; k_lrf8.hip).

Where a cloud runs under two pair scales and its slots share one kd-tree order, the second class
reads the Kw neighbours the first class found for every point, recomputes their exact keys under
its own scale, orders them and certifies against a stored lower bound that nothing outside the
list can be as near as its farthest entry; a wavefront that cannot is redone as a seeded one.
The bar is bitwise and needs no oracle: modes 0 (take) and 2 (every bound halved: every wavefront
redone) return what mode 1 (off: the seeded selection of DESIGN section 17) returns -- T, both
iteration counts, status and scaling_factor, and through the report entry the final match and
distance of every source point, which read every frame and normal.

Inputs are those of tests/test_gpu_lrf_seed.py: the five-scan chain S
(datasets.kitti_like_sequence(5, seed=4, n_az=200)), clouds cut from the bunny, integer lattices;
and a cloud with two point-symmetric clusters, whose centres see their neighbours in near-tied
pairs.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_TAKES = {"classes_taking": 0, "queries_taken": 0, "queries_redone": 0, "queries_failed": 0}


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
        self.total = int(self.src_off[-1])

    def args(self):
        return self.d_src.data_ptr(), self.src_off, self.d_tgt.data_ptr(), self.tgt_off


class Run:
    """One device batch through the report entry: results, every source point's final match and
    distance, and the call's graph, seed, take and kernel statistics."""

    def __init__(self, mod, batch, method, params, mode, device=0, stream=None, tree_sharing=0):
        import torch
        idx = torch.full((batch.total,), -2, dtype=torch.int32, device="cuda")
        dist = torch.zeros(batch.total, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        mod.set_lrf_taking(mode, device)
        mod.set_tree_sharing(tree_sharing, device)
        try:
            self.res, _ = mod.register_batch_report_device(
                *batch.args(), method, params, device=device, stream=stream.cuda_stream if stream else 0,
                max_correspondence_distance=1e9, corr_idx_ptr=idx.data_ptr(), corr_dist_ptr=dist.data_ptr())
            self.graph = mod.last_graph_stats(device)
            self.seed = mod.last_seed_stats(device)
            self.take = mod.last_take_stats(device)
            self.kt = mod.last_kernel_times(device)
        finally:
            mod.set_lrf_taking(0, device)
            mod.set_tree_sharing(0, device)
        if stream:
            stream.synchronize()
        torch.cuda.synchronize()
        self.idx, self.dist = idx.cpu().numpy(), dist.cpu().numpy()

    def same(self, other):
        return ([_bytes(r) for r in self.res] == [_bytes(r) for r in other.res] and
                np.array_equal(self.idx, other.idx) and self.dist.tobytes() == other.dist.tobytes())


def _modes(mod, parity_record, name, pairs, method, params, device=0, stream=None, batch=None):
    """Modes 0 and 2 against mode 1, bitwise; the graph statistics and the seeded classes of every
    mode are mode 1's, and every query of a seeded class is counted once.  Returns the runs."""
    batch = batch or DeviceBatch(pairs, stream)
    runs = {1: Run(mod, batch, method, params, 1, device=device, stream=stream)}
    assert (runs[1].idx >= 0).all()  # (every point has a match: the outputs were written)
    assert runs[1].take == NO_TAKES, runs[1].take
    for mode in (0, 2):
        r = runs[mode] = Run(mod, batch, method, params, mode, device=device, stream=stream)
        print(f"[lrf take] {name} mode {mode}: {r.take}; {r.seed}; hand-overs {r.kt['lrf_fallback']:.0f} "
              f"(mode 1: {runs[1].kt['lrf_fallback']:.0f}); lrf {r.kt['lrf_ms']:.3f} ms (mode 1: {runs[1].kt['lrf_ms']:.3f})")
        parity_record(f"lrf take: {name} mode {mode}", pairs=len(pairs), same=bool(r.same(runs[1])), **r.take)
        assert r.same(runs[1]), (name, mode)
        assert r.graph == runs[1].graph, (name, mode, r.graph, runs[1].graph)
        g = r.graph
        assert g["adopted"] == g["rejected_order"] == g["rejected_gap"] == g["no_list"] == 0
        assert r.seed["classes_seeded"] == runs[1].seed["classes_seeded"]
        assert r.seed["queries_seeded"] + r.seed["queries_unseeded"] == \
               runs[1].seed["queries_seeded"] + runs[1].seed["queries_unseeded"], (r.seed, runs[1].seed)
        assert r.seed["queries_failed"] == 0, r.seed
        # a taken query counts once, as a selected one does (the exact kernel counts its hand-overs again)
        assert r.kt["lrf_queries"] - r.kt["lrf_fallback"] == runs[1].kt["lrf_queries"] - runs[1].kt["lrf_fallback"], \
               (r.kt["lrf_queries"], r.kt["lrf_fallback"], runs[1].kt["lrf_queries"], runs[1].kt["lrf_fallback"])
        assert r.kt["lrf_fallback"] <= runs[1].kt["lrf_fallback"], (r.kt["lrf_fallback"], runs[1].kt["lrf_fallback"])
        assert r.take["classes_taking"] == runs[0].take["classes_taking"]
        assert r.take["queries_failed"] <= r.take["queries_redone"]
    return runs


# ------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("method", ["se3_gicp", "se3_pt2pl", "se3_gicp_with_cf"])
def test_chain(se3icp_mod, scans, parity_record, method):
    """Scan i+1 onto scan i over five scans: scans 2 and 3 run under two scales each, and their
    second classes take."""
    pairs = se3icp_mod.expand_edges(scans, se3icp_mod.sequence_edges(5))
    runs = _modes(se3icp_mod, parity_record, f"S {method}", pairs, method, se3icp_mod.kitti_params())
    n23 = scans[2].shape[0] + scans[3].shape[0]
    for mode in (0, 2):
        g, tk = runs[mode].graph, runs[mode].take
        assert tuple(g.values()) == (5, 8, 7, 7, 0, 0, 0, 0, 0), g
        assert tk["classes_taking"] == 2, tk
        assert tk["queries_taken"] + tk["queries_redone"] == n23, (tk, n23)
    assert runs[0].take["queries_failed"] == 0, runs[0].take
    assert runs[0].take["queries_taken"] > 0.9 * n23, runs[0].take  # (absent lists and partial waves are few)
    assert runs[2].take["queries_taken"] == 0 and runs[2].take["queries_redone"] == n23, runs[2].take


# ------------------------------------------------------------------ 2. a map: three takers of one source
def test_graph_map(se3icp_mod, scans, parity_record):
    """register_graph: scans 0, 1, 3 and 4 (enlarged by different factors) onto scan 2, whose
    radius is then the smallest, so it runs under four scales."""
    clouds = [np.ascontiguousarray(s * f) for s, f in zip(scans, (1.5, 1.4, 1.0, 1.3, 1.2))]
    edges = [(0, 2), (1, 2), (3, 2), (4, 2)]
    params = se3icp_mod.kitti_params()
    out = {}
    for mode in (1, 0, 2):
        se3icp_mod.set_lrf_taking(mode)
        try:
            res = se3icp_mod.register_graph(clouds, edges, "se3_gicp", params)
            out[mode] = ([_bytes(r) for r in res], se3icp_mod.last_graph_stats(), se3icp_mod.last_seed_stats(),
                         se3icp_mod.last_take_stats())
        finally:
            se3icp_mod.set_lrf_taking(0)
        print(f"[lrf take] map {mode}: {out[mode][1:]}")
    n2 = scans[2].shape[0]
    assert out[1][3] == NO_TAKES
    for mode in (0, 2):
        assert out[mode][0] == out[1][0], mode
        assert out[mode][1] == out[1][1], mode
        sd, tk = out[mode][2], out[mode][3]
        assert sd["classes_seeded"] == 3 and sd["queries_seeded"] + sd["queries_unseeded"] == 3 * n2, sd
        assert tk["classes_taking"] == 3 and tk["queries_taken"] + tk["queries_redone"] == 3 * n2, tk
    g = out[0][1]
    assert (g["clouds"], g["uses"], g["classes"], g["classes_full"]) == (5, 8, 8, 8), g
    assert out[0][3]["queries_failed"] == 0 and out[0][3]["queries_taken"] > 0.9 * 3 * n2, out[0][3]
    assert out[2][3]["queries_taken"] == 0, out[2][3]
    parity_record("lrf take: map", **out[0][3])


# ------------------------------------------------------------------ 3. ties
def _lattice(n, h):
    g = np.arange(n, dtype=np.float64) * h
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_ties_under_two_scales(se3icp_mod, parity_record):
    """Integer lattices: exact distance ties.  The first class hands such queries to the exact
    kernel and stores no list for them; a taking wavefront that meets one, or whose certificate
    finds the next point as near as its last, is redone."""
    clouds = [_lattice(11, 1.0), _lattice(12, 1.0), _lattice(10, 2.0)]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2), (0, 0)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=12)
    runs = _modes(se3icp_mod, parity_record, "ties", pairs, "se3_gicp", params)
    tk = runs[0].take
    assert tk["classes_taking"] > 0 and tk["queries_redone"] > 0, tk
    assert runs[0].kt["lrf_fallback"] > 0
    assert runs[2].take["queries_failed"] > 0, runs[2].take


def _symmetric_cluster(rng, centre, extra):
    """The centre, 100 pairs centre +- v, and `extra` unpaired points next to the centre: seen from
    the centre the ranks 1 + extra, 2 + extra, ... come in pairs at all but equal distances."""
    v = rng.normal(size=(100, 3)) * np.linspace(0.05, 1.0, 100)[:, None]
    pts = [centre[None, :], centre + v, centre - v]
    if extra:
        pts.append(centre + 0.01 * rng.normal(size=(extra, 3)))
    return np.concatenate(pts)


def test_gap_at_rounding_level(se3icp_mod, parity_record):
    """Two point-symmetric clusters whose centres see their neighbours in pairs p, 2 q - p that
    differ in distance at the f64 rounding level, one of them shifted by an extra point so that
    whatever the parity of Kw one centre has such a pair as its last kept and first dropped
    neighbour: the certificate's gap is far below its paddings, the wavefront is redone, and the
    result is the seeded selection's."""
    rng = np.random.default_rng(11)
    a = np.concatenate([_symmetric_cluster(rng, np.array([0.0, 0.0, 0.0]), 0),
                        _symmetric_cluster(rng, np.array([40.0, 3.0, -2.0]), 1),
                        rng.normal(size=(600, 3)) * 3.0 + np.array([20.0, 0.0, 0.0])])
    a = np.ascontiguousarray(a[rng.permutation(a.shape[0])])
    clouds = [np.ascontiguousarray(a * 1.7 + 0.5), a, np.ascontiguousarray(a[:900] * 0.6)]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1)])  # cloud 1 under two scales
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=3, max_num_iterations=8)
    runs = _modes(se3icp_mod, parity_record, "rounding-level gap", pairs, "se3_gicp", params)
    tk = runs[0].take
    assert tk["classes_taking"] == 1, tk
    assert tk["queries_failed"] >= 1 and tk["queries_redone"] >= 8, tk
    assert tk["queries_taken"] + tk["queries_redone"] == a.shape[0], tk
    assert tk["queries_taken"] > 0, tk


# ------------------------------------------------------------------ 4. structural sizes
@pytest.mark.parametrize("k", [30, 90, 127, 128, 150])
def test_small_clouds(se3icp_mod, bunny_clouds, parity_record, k):
    """7 .. 131 points: Kw = n, partial last waves, clouds of partial waves only; k at and over
    what the lists hold (Kw > 128 is redone whole)."""
    base = bunny_clouds[0]
    clouds = [np.ascontiguousarray(base[o:o + n] * (1.0 + 0.1 * i))
              for i, (o, n) in enumerate([(0, 7), (10, 8), (20, 9), (40, 64), (100, 65), (200, 90), (300, 91),
                                          (400, 92), (500, 131)])]
    edges = se3icp_mod.sequence_edges(len(clouds)) + [(0, 8), (8, 3)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=k, max_num_se3_iterations=3, max_num_iterations=8)
    pairs = se3icp_mod.expand_edges(clouds, edges)
    runs = _modes(se3icp_mod, parity_record, f"small k={k}", pairs, "se3_gicp", params)
    tk = runs[0].take
    assert tk["classes_taking"] > 0, tk
    assert tk["queries_taken"] + tk["queries_redone"] >= 7 * tk["classes_taking"], tk
    assert tk["queries_redone"] > 0, tk  # (the 7-point cloud is one partial wave)


def test_full_tree_nodes(se3icp_mod, bunny_unique, parity_record):
    """4,096 and 4,097 points: a full local tree node and one point over."""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])[:4097]], dtype=np.float64)
    clouds = [pts[:4096].copy(), pts * 1.3 + 0.01, pts[1:4097] * 0.8]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=10)
    runs = _modes(se3icp_mod, parity_record, "4096/4097", pairs, "se3_gicp", params)
    for mode in (0, 2):
        tk = runs[mode].take
        assert tk["classes_taking"] == 2 and tk["queries_taken"] + tk["queries_redone"] == 4096 + 4096, tk
    assert runs[0].take["queries_taken"] > 0.9 * 8192, runs[0].take


# ------------------------------------------------------------------ 5. other paths
CHAIN_B = [(1, 0), (2, 1), (3, 1), (1, 1)]


def test_tree_sharing_off(se3icp_mod, bunny_clouds):
    """Without one tree order per cloud a tree slot means another point in every class: nothing
    takes, the statistics are 0 and the results are equal."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    batch = DeviceBatch(se3icp_mod.expand_edges(bunny_clouds, CHAIN_B))
    want = Run(se3icp_mod, batch, "se3_gicp", params, 1)
    took = Run(se3icp_mod, batch, "se3_gicp", params, 0)
    assert took.take["classes_taking"] > 0 and took.same(want)
    for mode in (0, 1, 2):
        got = Run(se3icp_mod, batch, "se3_gicp", params, mode, tree_sharing=1)
        assert got.same(want), mode
        assert got.take == NO_TAKES, got.take
        assert got.seed["classes_seeded"] == want.seed["classes_seeded"] > 0


@pytest.mark.parametrize("exact", [1, 2])
def test_lrf_exact_modes(se3icp_mod, bunny_clouds, exact):
    """se3icp_set_lrf_exact: every class through the selected exact kernel, nothing takes."""
    from se3icp import registration
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    batch = DeviceBatch(se3icp_mod.expand_edges(bunny_clouds, CHAIN_B))
    want = Run(se3icp_mod, batch, "se3_gicp", params, 1)
    registration.set_lrf_exact(exact)
    try:
        for mode in (0, 1, 2):
            got = Run(se3icp_mod, batch, "se3_gicp", params, mode)
            assert got.same(want), mode
            assert got.take == NO_TAKES, got.take
            assert got.graph == want.graph
    finally:
        registration.set_lrf_exact(0)


@pytest.mark.parametrize("seeding", [1, 2, 3])
def test_seeding_modes_do_not_take(se3icp_mod, bunny_clouds, seeding):
    """Seeding off or in a diagnostic mode: the seeded selection runs as before, nothing takes."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    batch = DeviceBatch(se3icp_mod.expand_edges(bunny_clouds, CHAIN_B))
    want = Run(se3icp_mod, batch, "se3_gicp", params, 1)
    se3icp_mod.set_lrf_seeding(seeding)
    try:
        got = Run(se3icp_mod, batch, "se3_gicp", params, 0)
    finally:
        se3icp_mod.set_lrf_seeding(0)
    assert got.same(want) and got.take == NO_TAKES, got.take


def test_engine_slot_stream_and_host_batch(se3icp_mod, bunny_clouds, parity_record):
    """A further engine of the same GPU (device | slot << 8) whose first call takes, the switch
    being that engine's; calls on the caller's stream; a host batch right after a taking call."""
    import torch
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    slot1 = 0 | 1 << 8
    r1 = _modes(se3icp_mod, parity_record, "slot 1", pairs, "se3_gicp", params, device=slot1)
    r0 = _modes(se3icp_mod, parity_record, "slot 0", pairs, "se3_gicp", params)
    assert r0[0].take["classes_taking"] > 0 and r0[0].take["queries_taken"] > 0
    for mode in (0, 2):
        assert r1[mode].same(r0[1]) and r1[mode].take == r0[mode].take
    # slot 1 switched off does not switch slot 0 off
    se3icp_mod.set_lrf_taking(1, slot1)
    try:
        batch = DeviceBatch(pairs)
        se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params)
        assert se3icp_mod.last_take_stats() == r0[0].take
        se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params, device=slot1)
        assert se3icp_mod.last_take_stats(slot1) == NO_TAKES
    finally:
        se3icp_mod.set_lrf_taking(0, slot1)
    # a host batch right after: it takes nothing and returns the device batch's results
    host = se3icp_mod.register_batch(pairs, "se3_gicp", params)
    assert [_bytes(r) for r in host] == [_bytes(r) for r in r0[1].res]
    assert se3icp_mod.last_take_stats() == NO_TAKES
    stream = torch.cuda.Stream()
    rs = _modes(se3icp_mod, parity_record, "stream", pairs, "se3_gicp", params, stream=stream)
    for mode in (0, 2):
        assert rs[mode].same(r0[1]) and rs[mode].take == r0[mode].take


def test_nothing_shared(se3icp_mod, bunny_clouds, parity_record):
    """Distinct clouds (equal point counts: hashed, no hash agrees), and clouds that share but
    under one scale each: nothing takes and the selection does what mode 1 does."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=5, max_num_iterations=20)
    c = bunny_clouds
    distinct = [(c[0][:3000], c[1][:3000]), (c[2][:3000], c[3][:3000])]
    one_scale = [(c[0], c[1]), (c[0], c[1])]
    for name, pairs in [("distinct", distinct), ("one scale", one_scale)]:
        runs = _modes(se3icp_mod, parity_record, f"nothing shared {name}", pairs, "se3_gicp", params)
        for mode in (0, 2):
            assert runs[mode].take == NO_TAKES, (name, mode, runs[mode].take)
            assert (runs[mode].kt["lrf_queries"], runs[mode].kt["lrf_fallback"]) == \
                   (runs[1].kt["lrf_queries"], runs[1].kt["lrf_fallback"])
