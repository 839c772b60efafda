"""GPU tests of one kd-tree order per cloud (se3icp_set_tree_sharing, se3icp_last_tree_stats;
k_tree.hip).

Where several slots of a call hold one confirmed cloud, only the first builds its 3-D and 12-D
trees; the later slots take its finished order and compute their own tree-ordered vectors and
boxes.  No result depends on a tree's order, so the bar is bitwise and needs no oracle: mode 0
(adopt) returns what mode 1 (every slot builds) returns, and mode 1 what batch sharing level 1
(the plain batch) returns -- T, both iteration counts, status and scaling_factor, and through
the report entry the final match and distance of every source point.  The tree statistics say
what was built and what adopted.

Tree quality is not left to timing: on the chain cases the loop's device-counted distance
evaluations and box tests of mode 0 stay under 1.5 x mode 1's (an adopter whose boxes came from
the wrong vectors, or whose order is scrambled, prunes nothing), and both are printed and
recorded.

Shapes: the smallest at which each path of the build can go wrong (tree.hpp: leaves of 64
points, level-G nodes of 4,096, the multi-pass levels below 32 (3-D) / 64 (12-D) nodes).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WORK = ("se3_dist_evals", "se3_box_tests", "r3_dist_evals", "r3_box_tests")
WORK_CAP = 1.5  # mode 0's loop NN work against mode 1's


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


def _scans(n, n_az):
    from se3icp import datasets
    s, _ = datasets.kitti_like_sequence(n, seed=4, n_az=n_az)
    return [np.ascontiguousarray(x, dtype=np.float64) for x in s]


@pytest.fixture(scope="module")
def scans5():
    """The five-scan chain S of the sharing and seeding tests (~12,500 points a scan)."""
    return _scans(5, 200)


@pytest.fixture(scope="module")
def scans16():
    """Sixteen scans of 8,440 .. 8,530 points: two global levels (G = 2)."""
    s = _scans(16, 135)
    assert all(8192 < x.shape[0] <= 16384 for x in s)
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
        self.slots = 2 * len(pairs)

    def args(self):
        return self.d_src.data_ptr(), self.src_off, self.d_tgt.data_ptr(), self.tgt_off


class Run:
    """One device batch through the report entry: results, every source point's final match and
    distance, and the call's tree, graph, seed and kernel statistics."""

    def __init__(self, mod, batch, method, params, mode, level=0, device=0, stream=None):
        import torch
        idx = torch.full((batch.total,), -2, dtype=torch.int32, device="cuda")
        dist = torch.zeros(batch.total, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        mod.set_batch_sharing(level, device)
        mod.set_tree_sharing(mode, device)
        try:
            self.res, _ = mod.register_batch_report_device(
                *batch.args(), method, params, device=device, stream=stream.cuda_stream if stream else 0,
                max_correspondence_distance=1e9, corr_idx_ptr=idx.data_ptr(), corr_dist_ptr=dist.data_ptr())
            self.tree = mod.last_tree_stats(device)
            self.graph = mod.last_graph_stats(device) if level != 1 else None
            self.seed = mod.last_seed_stats(device)
            self.kt = mod.last_kernel_times(device)
        finally:
            mod.set_batch_sharing(0, device)
            mod.set_tree_sharing(0, device)
        if stream:
            stream.synchronize()
        torch.cuda.synchronize()
        self.idx, self.dist = idx.cpu().numpy(), dist.cpu().numpy()

    def same(self, other):
        return ([_bytes(r) for r in self.res] == [_bytes(r) for r in other.res] and
                np.array_equal(self.idx, other.idx) and self.dist.tobytes() == other.dist.tobytes())


def _tree(b3, a3, b12, a12):
    return {"built_3d": b3, "adopted_3d": a3, "built_12d": b12, "adopted_12d": a12}


def _modes(mod, parity_record, name, pairs, method, params, clouds, device=0, stream=None, batch=None, work=False):
    """Mode 0 against mode 1, mode 1 against sharing level 1, all bitwise, and the tree statistics:
    `clouds` distinct clouds in the batch's slots.  work: the loop's NN work counters of mode 0
    stay under WORK_CAP x mode 1's.  Returns the runs (0, 1, "plain")."""
    batch = batch or DeviceBatch(pairs, stream)
    U = batch.slots
    se3 = method.startswith("se3")
    runs = {"plain": Run(mod, batch, method, params, 0, level=1, device=device, stream=stream),
            1: Run(mod, batch, method, params, 1, device=device, stream=stream),
            0: Run(mod, batch, method, params, 0, device=device, stream=stream)}
    assert (runs[1].idx >= 0).all()  # (every point has a match: the outputs were written)
    assert runs[1].same(runs["plain"]), name
    assert runs[0].same(runs[1]), name
    every = _tree(U, 0, U if se3 else 0, 0)
    assert runs["plain"].tree == every and runs[1].tree == every, (runs["plain"].tree, runs[1].tree)
    assert runs[0].tree == _tree(clouds, U - clouds, clouds if se3 else 0, U - clouds if se3 else 0), (name, runs[0].tree)
    # sharing the trees changes neither the classes nor which of them are seeded (a seeded
    # class's wavefronts are cut from its tree order, so how many of them meet an absent seed
    # may differ; every query of a seeded class is still counted once)
    assert runs[0].graph == runs[1].graph, name
    s0, s1 = runs[0].seed, runs[1].seed
    assert s0["classes_seeded"] == s1["classes_seeded"] and s0["queries_failed"] == s1["queries_failed"] == 0, (s0, s1)
    assert s0["queries_seeded"] + s0["queries_unseeded"] == s1["queries_seeded"] + s1["queries_unseeded"], (s0, s1)
    g = runs[0].graph
    assert g["adopted"] == g["rejected_order"] == g["rejected_gap"] == g["no_list"] == 0
    ratios = {}
    for k in WORK:
        a, b = runs[0].kt[k], runs[1].kt[k]
        ratios[k] = a / b if b > 0 else 1.0
        print(f"[tree adopt] {name} {k}: mode 0 {a:.0f} mode 1 {b:.0f} ratio {ratios[k]:.4f}")
    parity_record(f"tree adopt: {name}", pairs=len(pairs), same=True, **runs[0].tree,
                  **{f"{k}_mode0": runs[0].kt[k] for k in WORK}, **{f"{k}_mode1": runs[1].kt[k] for k in WORK})
    if work:
        for k in WORK:
            assert runs[0].kt[k] <= WORK_CAP * runs[1].kt[k], (name, k, runs[0].kt[k], runs[1].kt[k])
    return runs


def _chain(mod, scans):
    return mod.expand_edges(scans, mod.sequence_edges(len(scans)))


def _quick(mod, **kw):
    return mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=10, **kw)


# ------------------------------------------------------------------ 1. the five-scan chain, every method
@pytest.mark.parametrize("method", ["se3_gicp", "se3_pt2pl", "se3_gicp_with_cf", "gicp"])
def test_chain_methods(se3icp_mod, scans5, parity_record, method):
    """Scan i+1 onto scan i: scans 1, 2 and 3 lie in two slots each.  gicp has 3-D trees only."""
    runs = _modes(se3icp_mod, parity_record, f"S {method}", _chain(se3icp_mod, scans5), method,
                  se3icp_mod.kitti_params(), clouds=5, work=True)
    if method == "gicp":
        assert runs[0].tree == _tree(5, 3, 0, 0)


# ------------------------------------------------------------------ 2. leaves and the first split
def test_small_clouds(se3icp_mod, bunny_clouds, parity_record):
    """Clouds of 7, 64 and 65 points alone (L = 0: no level, k_tree_finish; L = 1: the first
    split) and beside each other."""
    base = bunny_clouds[0]
    c7, c64, c65 = (np.ascontiguousarray(base[o:o + n] * f) for o, n, f in [(0, 7, 1.0), (40, 64, 1.1), (100, 65, 1.2)])
    d7, d64, d65 = (np.ascontiguousarray(base[o:o + n] * f) for o, n, f in [(200, 7, 1.3), (300, 64, 0.9), (400, 65, 0.8)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=3, max_num_iterations=8)
    for name, cl in [("7", [c7, d7, c7 * 1.5]), ("64", [c64, d64, c64 * 1.5]), ("65", [c65, d65, c65 * 1.5]),
                     ("7/64/65", [c7, c64, c65])]:
        # a triangle: every cloud is once a source and once a target
        pairs = se3icp_mod.expand_edges(cl, [(1, 0), (2, 1), (0, 2)])
        _modes(se3icp_mod, parity_record, f"small {name}", pairs, "se3_gicp", params, clouds=3)


# ------------------------------------------------------------------ 3. G goes 0 -> 1
def test_full_local_node(se3icp_mod, bunny_unique, parity_record):
    """4,096 points: one full level-G node, no global level; 4,097: the first global level."""
    rng = np.random.default_rng(3)
    pts = np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])[:4097]], dtype=np.float64)
    a, b = pts[:4096].copy(), np.ascontiguousarray(pts[1:4097] * 0.8)
    for name, cl in [("4096", [a, np.ascontiguousarray(a[::-1] * 1.3 + 0.01), b]),
                     ("4097", [a, np.ascontiguousarray(pts * 1.3 + 0.01), b])]:
        pairs = se3icp_mod.expand_edges(cl, [(1, 0), (2, 1), (0, 2)])
        _modes(se3icp_mod, parity_record, f"node {name}", pairs, "se3_gicp", _quick(se3icp_mod), clouds=3)


# ------------------------------------------------------------------ 4. global levels
def test_multipass_levels(se3icp_mod, scans16, parity_record):
    """Four scans in a chain: G = 2 and four builders, so both global levels take the multi-pass
    k_part_* path, whose passes over all points skip the adopters'."""
    _modes(se3icp_mod, parity_record, "G2 multipass", _chain(se3icp_mod, scans16[:4]), "se3_gicp", _quick(se3icp_mod),
           clouds=4, work=True)


def test_level_kernel(se3icp_mod, scans16, parity_record):
    """Sixteen scans in a chain: level 1 of the 3-D build has 32 builder nodes and is one
    k_tree_level launch over the builders' list; the 12-D levels stay multi-pass."""
    _modes(se3icp_mod, parity_record, "G2 level kernel", _chain(se3icp_mod, scans16), "se3_gicp", _quick(se3icp_mod),
           clouds=16, work=True)


def test_small_beside_large(se3icp_mod, bunny_clouds, parity_record):
    """G comes from the largest cloud: the level-G nodes of a 1,200-point pair beside chains of
    ~9,400 points are nearly empty, builders' and adopters' alike."""
    big = _scans(3, 150)
    small = [np.ascontiguousarray(bunny_clouds[0][:1200]), np.ascontiguousarray(bunny_clouds[1][:1200])]
    pairs = ([(small[0], small[1])] + _chain(se3icp_mod, big) + [(small[1], small[0])])
    _modes(se3icp_mod, parity_record, "small beside large", pairs, "se3_gicp", _quick(se3icp_mod), clouds=5, work=True)


# ------------------------------------------------------------------ 5. a map: adopted target trees
def test_graph_map(se3icp_mod, scans5, parity_record):
    """register_graph, scans 0, 1, 3 and 4 onto scan 2: one donor, three adopters that are targets,
    so full 12-D trees with boxes are adopted under other scales."""
    clouds = [np.ascontiguousarray(s * f) for s, f in zip(scans5, (1.5, 1.4, 1.0, 1.3, 1.2))]
    edges = [(0, 2), (1, 2), (3, 2), (4, 2)]
    params = se3icp_mod.kitti_params()
    out = {}
    for key, mode, sharing in [("plain", 0, 1), (1, 1, 0), (0, 0, 0)]:
        se3icp_mod.set_tree_sharing(mode)
        try:
            res, rep = se3icp_mod.register_graph_report(clouds, edges, "se3_gicp", params, sharing=sharing,
                                                        max_correspondence_distance=1e9, per_point=True)
            out[key] = ([_bytes(r) for r in res], [(p.corr_idx.tobytes(), p.corr_dist.tobytes()) for p in rep],
                        se3icp_mod.last_tree_stats(), se3icp_mod.last_graph_stats(), se3icp_mod.last_kernel_times())
        finally:
            se3icp_mod.set_tree_sharing(0)
    assert len(set(out["plain"][0])) == 4
    for key in (1, 0):
        assert out[key][0] == out["plain"][0] and out[key][1] == out["plain"][1], key
    assert out["plain"][2] == _tree(8, 0, 8, 0) and out[1][2] == _tree(8, 0, 8, 0)
    assert out[0][2] == _tree(5, 3, 5, 3), out[0][2]
    assert out[0][3] == out[1][3]
    for k in WORK:
        a, b = out[0][4][k], out[1][4][k]
        print(f"[tree adopt] map {k}: mode 0 {a:.0f} mode 1 {b:.0f} ratio {a / b if b else 1.0:.4f}")
        assert a <= WORK_CAP * b, (k, a, b)
    parity_record("tree adopt: map", **out[0][2], **{f"{k}_mode0": out[0][4][k] for k in WORK},
                  **{f"{k}_mode1": out[1][4][k] for k in WORK})


# ------------------------------------------------------------------ 6. ties
def _lattice(n, h):
    g = np.arange(n, dtype=np.float64) * h
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def test_ties_under_two_scales(se3icp_mod, parity_record):
    """Integer lattices under two scales: split keys tie, and the donor's order is not the one
    the adopter's own build finds."""
    clouds = [_lattice(11, 1.0), _lattice(12, 1.0), _lattice(10, 2.0)]
    pairs = se3icp_mod.expand_edges(clouds, [(1, 0), (2, 1), (0, 2), (0, 0)])
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=12)
    _modes(se3icp_mod, parity_record, "ties", pairs, "se3_gicp", params, clouds=3)


# ------------------------------------------------------------------ 7. nothing to share
def test_nothing_shared(se3icp_mod, bunny_clouds, parity_record):
    """Distinct clouds of equal point counts (hashed, no hash agrees): every tree is built, and the
    kernels do the work of mode 1."""
    params = se3icp_mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=5, max_num_iterations=20)
    c = bunny_clouds
    pairs = [(c[0][:3000], c[1][:3000]), (c[2][:3000], c[3][:3000])]
    runs = _modes(se3icp_mod, parity_record, "nothing shared", pairs, "se3_gicp", params, clouds=4)
    assert runs[0].tree == _tree(4, 0, 4, 0)
    for k in WORK + ("lrf_queries", "lrf_fallback", "lrf_leaves", "lrf_box_tests", "lrf_candidates"):
        assert runs[0].kt[k] == runs[1].kt[k], (k, runs[0].kt[k], runs[1].kt[k])


# ------------------------------------------------------------------ 8. other paths
CHAIN_B = [(1, 0), (2, 1), (3, 1), (1, 1)]


@pytest.mark.parametrize("exact", [1, 2])
def test_lrf_exact_modes(se3icp_mod, bunny_clouds, parity_record, exact):
    """se3icp_set_lrf_exact: the exact selection kernels walk the adopted 3-D trees too."""
    from se3icp import registration
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    batch = DeviceBatch(pairs)
    want = Run(se3icp_mod, batch, "se3_gicp", params, 1)
    registration.set_lrf_exact(exact)
    try:
        runs = _modes(se3icp_mod, parity_record, f"lrf exact {exact}", pairs, "se3_gicp", params, clouds=4, batch=batch)
        assert runs[0].same(want)
    finally:
        registration.set_lrf_exact(0)


def test_engine_slot_stream_and_host_batch(se3icp_mod, bunny_clouds, parity_record):
    """A further engine of the same GPU (device | slot << 8) whose first call adopts; the switch
    is the engine's; calls on the caller's stream; and a host batch right after an adopting call
    adopts nothing."""
    import torch
    params = se3icp_mod.default_params(number_of_nn_for_LRF=60)
    pairs = se3icp_mod.expand_edges(bunny_clouds, CHAIN_B)
    slot1 = 0 | 1 << 8
    r1 = _modes(se3icp_mod, parity_record, "slot 1", pairs, "se3_gicp", params, clouds=4, device=slot1)
    r0 = _modes(se3icp_mod, parity_record, "slot 0", pairs, "se3_gicp", params, clouds=4)
    assert r1[0].same(r0[1])
    # slot 1 switched off does not switch slot 0 off
    se3icp_mod.set_tree_sharing(1, slot1)
    try:
        batch = DeviceBatch(pairs)
        se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params)
        assert se3icp_mod.last_tree_stats() == _tree(4, 4, 4, 4)
        se3icp_mod.register_batch_device(*batch.args(), "se3_gicp", params, device=slot1)
        assert se3icp_mod.last_tree_stats(slot1) == _tree(8, 0, 8, 0)
    finally:
        se3icp_mod.set_tree_sharing(0, slot1)
    stream = torch.cuda.Stream()
    rs = _modes(se3icp_mod, parity_record, "stream", pairs, "se3_gicp", params, clouds=4, stream=stream)
    assert rs[0].same(r0[1])
    # the host-pointer entry does not look for shared clouds: its trees are all built, and its
    # results are the device batch's
    host = se3icp_mod.register_batch(pairs, "se3_gicp", params)
    assert se3icp_mod.last_tree_stats() == _tree(8, 0, 8, 0)
    assert [_bytes(r) for r in host] == [_bytes(r) for r in r0[1].res]
