"""GPU tests of seeding a cloud's later classes from its first class's neighbour distances
(se3icp_set_lrf_seeding, se3icp_last_seed_stats; k_lrf8.hip).

Where a cloud runs under two pair scales, its second class starts the selection of every
wavefront from the bound the first class's Kw-th neighbour distance gives, collects what lies
within it and certifies itself with one closing tightening.  The seed is a hint; the bar is
bitwise and needs no oracle: modes 0 (seeded), 2 (every seed halved: the certificate fails and
the exact kernel takes the queries) and 3 (every seed times 4: loose seeds, overflowing lists)
return what mode 1 (off) returns -- T, both iteration counts, status and scaling_factor, and
through the report entry the final match and distance of every source point, which read every
frame and normal -- and mode 1 returns what se3icp_set_batch_sharing level 1 (the plain batch)
returns.  se3icp_last_graph_stats keeps its values: a seeded class ran a full selection.

Inputs are those of tests/test_gpu_batch_sharing.py: the five-scan chain S
(datasets.kitti_like_sequence(5, seed=4, n_az=200)), clouds cut from the bunny, integer lattices.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = (0, 2, 3)


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
    distance, and the call's graph, seed and kernel statistics."""

    def __init__(self, mod, batch, method, params, mode, level=0, device=0, stream=None):
        import torch
        idx = torch.full((batch.total,), -2, dtype=torch.int32, device="cuda")
        dist = torch.zeros(batch.total, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        mod.set_batch_sharing(level, device)
        mod.set_lrf_seeding(mode, device)
        try:
            self.res, _ = mod.register_batch_report_device(
                *batch.args(), method, params, device=device, stream=stream.cuda_stream if stream else 0,
                max_correspondence_distance=1e9, corr_idx_ptr=idx.data_ptr(), corr_dist_ptr=dist.data_ptr())
            self.graph = mod.last_graph_stats(device) if level != 1 else None
            self.seed = mod.last_seed_stats(device)
            self.kt = mod.last_kernel_times(device)
        finally:
            mod.set_batch_sharing(0, device)
            mod.set_lrf_seeding(0, device)
        if stream:
            stream.synchronize()
        torch.cuda.synchronize()
        self.idx, self.dist = idx.cpu().numpy(), dist.cpu().numpy()

    def same(self, other):
        return ([_bytes(r) for r in self.res] == [_bytes(r) for r in other.res] and
                np.array_equal(self.idx, other.idx) and self.dist.tobytes() == other.dist.tobytes())


NO_SEEDS = {"classes_seeded": 0, "queries_seeded": 0, "queries_unseeded": 0, "queries_failed": 0}


def _modes(mod, parity_record, name, pairs, method, params, device=0, stream=None, batch=None):
    """Modes 0, 2 and 3 against mode 1, mode 1 against sharing level 1, all bitwise; the graph
    statistics of every mode are mode 1's.  Returns the runs by mode (and "plain": level 1)."""
    batch = batch or DeviceBatch(pairs, stream)
    runs = {"plain": Run(mod, batch, method, params, 1, level=1, device=device, stream=stream),
            1: Run(mod, batch, method, params, 1, device=device, stream=stream)}
    assert (runs[1].idx >= 0).all()  # (every point has a match: the outputs were written)
    assert runs[1].same(runs["plain"]), name
    assert runs[1].seed == NO_SEEDS and runs["plain"].seed == NO_SEEDS, (runs[1].seed, runs["plain"].seed)
    for mode in MODES:
        r = runs[mode] = Run(mod, batch, method, params, mode, device=device, stream=stream)
        print(f"[lrf seed] {name} mode {mode}: {r.seed}; hand-overs {r.kt['lrf_fallback']:.0f} "
              f"(mode 1: {runs[1].kt['lrf_fallback']:.0f}); lrf {r.kt['lrf_ms']:.3f} ms (mode 1: {runs[1].kt['lrf_ms']:.3f})")
        parity_record(f"lrf seed: {name} mode {mode}", pairs=len(pairs), same=bool(r.same(runs[1])), **r.seed)
        assert r.same(runs[1]), (name, mode)
        assert r.graph == runs[1].graph, (name, mode, r.graph, runs[1].graph)
        g = r.graph
        assert g["adopted"] == g["rejected_order"] == g["rejected_gap"] == g["no_list"] == 0
        if mode == 0:
            # correct seeds never fail; a seeded wave's closing bound keeps a subset of what the
            # unseeded wave's last bound keeps, so it hands over no more queries
            assert r.seed["queries_failed"] == 0, r.seed
            assert r.kt["lrf_fallback"] <= runs[1].kt["lrf_fallback"], (r.kt["lrf_fallback"], runs[1].kt["lrf_fallback"])
        if mode == 3:
            assert r.seed["queries_failed"] == 0, r.seed
        assert r.seed["classes_seeded"] == runs[0].seed["classes_seeded"]
    return runs


# ------------------------------------------------------------------ 1. the chain
@pytest.mark.parametrize("method", ["se3_gicp", "se3_pt2pl", "se3_gicp_with_cf"])
def test_chain(se3icp_mod, scans, parity_record, method):
    """Scan i+1 onto scan i over five scans: scans 2 and 3 run under two scales each."""
    pairs = se3icp_mod.expand_edges(scans, se3icp_mod.sequence_edges(5))
    runs = _modes(se3icp_mod, parity_record, f"S {method}", pairs, method, se3icp_mod.kitti_params())
    n23 = scans[2].shape[0] + scans[3].shape[0]
    for mode in MODES:
        g, sd = runs[mode].graph, runs[mode].seed
        assert tuple(g.values()) == (5, 8, 7, 7, 0, 0, 0, 0, 0), g
        assert sd["classes_seeded"] == 2, sd
        assert sd["queries_seeded"] + sd["queries_unseeded"] == n23, (sd, n23)
    assert runs[0].seed["queries_failed"] == 0 and runs[3].seed["queries_failed"] == 0
    assert runs[0].seed["queries_seeded"] > 0.9 * n23, runs[0].seed  # (hand-overs of the first class are few)
    assert runs[2].seed["queries_failed"] > 0, runs[2].seed
    assert runs[2].seed["queries_failed"] <= runs[2].seed["queries_seeded"]


# ------------------------------------------------------------------ 2. a map: three and more classes of one cloud
def test_graph_map(se3icp_mod, scans, parity_record):
    """register_graph: scans 0, 1, 3 and 4 (enlarged by different factors) onto scan 2, whose
    radius is then the smallest, so it runs under four scales."""
    clouds = [np.ascontiguousarray(s * f) for s, f in zip(scans, (1.5, 1.4, 1.0, 1.3, 1.2))]
    edges = [(0, 2), (1, 2), (3, 2), (4, 2)]
    params = se3icp_mod.kitti_params()
    out = {}
    for key, mode, sharing in [("plain", 1, 1), (1, 1, 0), (0, 0, 0), (2, 2, 0), (3, 3, 0)]:
        se3icp_mod.set_lrf_seeding(mode)
        try:
            res = se3icp_mod.register_graph(clouds, edges, "se3_gicp", params, sharing=sharing)
            out[key] = ([_bytes(r) for r in res], se3icp_mod.last_graph_stats(), se3icp_mod.last_seed_stats())
        finally:
            se3icp_mod.set_lrf_seeding(0)
        print(f"[lrf seed] map {key}: {out[key][1]} {out[key][2]}")
    assert len(set(out["plain"][0])) == 4
    for key in (1, 0, 2, 3):
        assert out[key][0] == out["plain"][0], key
        assert out[key][1] == out[1][1], key
    assert out["plain"][2] == NO_SEEDS and out[1][2] == NO_SEEDS
    g = out[0][1]
    assert (g["clouds"], g["uses"], g["classes"], g["classes_full"]) == (5, 8, 8, 8), g
    n2 = scans[2].shape[0]
    for mode in MODES:
        sd = out[mode][2]
        assert sd["classes_seeded"] == 3 and sd["queries_seeded"] + sd["queries_unseeded"] == 3 * n2, sd
    assert out[0][2]["queries_failed"] == 0 and out[3][2]["queries_failed"] == 0 and out[2][2]["queries_failed"] > 0
    parity_record("lrf seed: map", **out[0][2])


# ------------------------------------------------------------------ 3. ties
def _lattice(n, h):
    g = np.arange(n, dtype=np.float64) * h
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_ties_under_two_scales(se3icp_mod, parity_record):
    """Integer lattices: exact distance ties hand queries to the exact kernel in the first class
    (absent seeds) and in the seeded one."""
    clouds = [_lattice(11, 1.0), _lattice(12, 1.0), _lattice(10, 2.0)]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2), (0, 0)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=12)
    runs = _modes(se3icp_mod, parity_record, "ties", pairs, "se3_gicp", params)
    assert runs[0].seed["classes_seeded"] > 0 and runs[0].kt["lrf_fallback"] > 0


# ------------------------------------------------------------------ 4. structural sizes
@pytest.mark.parametrize("k", [30, 90, 127, 128, 150])
def test_small_clouds(se3icp_mod, bunny_clouds, parity_record, k):
    """7 .. 131 points: Kw = n, partial last waves, clouds of partial waves only; k at and over
    what the LDS kernels hold."""
    base = bunny_clouds[0]
    clouds = [np.ascontiguousarray(base[o:o + n] * (1.0 + 0.1 * i))
              for i, (o, n) in enumerate([(0, 7), (10, 8), (20, 9), (40, 64), (100, 65), (200, 90), (300, 91),
                                          (400, 92), (500, 131)])]
    edges = se3icp_mod.sequence_edges(len(clouds)) + [(0, 8), (8, 3)]
    params = se3icp_mod.default_params(number_of_nn_for_LRF=k, max_num_se3_iterations=3, max_num_iterations=8)
    pairs = se3icp_mod.expand_edges(clouds, edges)
    runs = _modes(se3icp_mod, parity_record, f"small k={k}", pairs, "se3_gicp", params)
    sd = runs[0].seed
    assert sd["classes_seeded"] > 0, sd
    # every query of a seeded class is counted once, whichever way its wave went
    assert sd["queries_seeded"] + sd["queries_unseeded"] >= 7 * sd["classes_seeded"], sd


def test_full_tree_nodes(se3icp_mod, bunny_unique, parity_record):
    """4,096 and 4,097 points: a full local tree node and one point over."""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])[:4097]], dtype=np.float64)
    clouds = [pts[:4096].copy(), pts * 1.3 + 0.01, pts[1:4097] * 0.8]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=10)
    runs = _modes(se3icp_mod, parity_record, "4096/4097", pairs, "se3_gicp", params)
    g = runs[0].graph
    assert (g["clouds"], g["classes"]) == (3, 5), g  # clouds 0 and 2 run under two scales each
    for mode in MODES:
        sd = runs[mode].seed
        assert sd["classes_seeded"] == 2 and sd["queries_seeded"] + sd["queries_unseeded"] == 4096 + 4096, sd


# ------------------------------------------------------------------ 5. other paths
CHAIN_B = [(1, 0), (2, 1), (3, 1), (1, 1)]


@pytest.mark.parametrize("exact", [1, 2])
def test_lrf_exact_modes(se3icp_mod, bunny_clouds, exact):
    """se3icp_set_lrf_exact: every class through the selected exact kernel, nothing is seeded."""
    from se3icp import registration
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    batch = DeviceBatch(pairs)
    want = Run(se3icp_mod, batch, "se3_gicp", params, 1)
    registration.set_lrf_exact(exact)
    try:
        for mode in (0, 1, 2, 3):
            got = Run(se3icp_mod, batch, "se3_gicp", params, mode)
            assert got.same(want), mode
            assert got.seed == NO_SEEDS, got.seed
            assert got.graph == want.graph
    finally:
        registration.set_lrf_exact(0)


def test_engine_slot_and_callers_stream(se3icp_mod, bunny_clouds, parity_record):
    """A further engine of the same GPU (device | slot << 8) whose first call seeds, and calls on
    the caller's stream; the switch is the engine's."""
    import torch
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    slot1 = 0 | 1 << 8
    r1 = _modes(se3icp_mod, parity_record, "slot 1", pairs, "se3_gicp", params, device=slot1)
    r0 = _modes(se3icp_mod, parity_record, "slot 0", pairs, "se3_gicp", params)
    assert r0[0].seed["classes_seeded"] > 0
    for mode in MODES:
        assert r1[mode].same(r0[1]) and r1[mode].seed["classes_seeded"] == r0[mode].seed["classes_seeded"]
    # slot 1 switched off does not switch slot 0 off
    se3icp_mod.set_lrf_seeding(1, slot1)
    try:
        batch = DeviceBatch(pairs)
        se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params)
        assert se3icp_mod.last_seed_stats()["classes_seeded"] == r0[0].seed["classes_seeded"]
        se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params, device=slot1)
        assert se3icp_mod.last_seed_stats(slot1) == NO_SEEDS
    finally:
        se3icp_mod.set_lrf_seeding(0, slot1)
    stream = torch.cuda.Stream()
    rs = _modes(se3icp_mod, parity_record, "stream", pairs, "se3_gicp", params, stream=stream)
    for mode in MODES:
        assert rs[mode].same(r0[1]) and rs[mode].seed == r0[mode].seed


def test_nothing_shared(se3icp_mod, bunny_clouds, parity_record):
    """Distinct clouds (equal point counts: hashed, no hash agrees), and clouds that share but
    under one scale each: nothing is seeded and the selection does what mode 1 does."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=5, max_num_iterations=20)
    c = bunny_clouds
    distinct = [(c[0][:3000], c[1][:3000]), (c[2][:3000], c[3][:3000])]
    one_scale = [(c[0], c[1]), (c[0], c[1])]
    for name, pairs in [("distinct", distinct), ("one scale", one_scale)]:
        runs = _modes(se3icp_mod, parity_record, f"nothing shared {name}", pairs, "se3_gicp", params)
        for mode in MODES:
            assert runs[mode].seed == NO_SEEDS, (name, mode, runs[mode].seed)
            assert (runs[mode].kt["lrf_queries"], runs[mode].kt["lrf_fallback"]) == \
                   (runs[1].kt["lrf_queries"], runs[1].kt["lrf_fallback"])
