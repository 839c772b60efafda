"""GPU tests of the kd-trees themselves (se3icp_set_tree_record; k_tree.hip).

Every search of the engine prunes on the node boxes, and every exactness claim rests on them.
Here the trees a call built are read back -- order, tree-ordered vectors, every node box -- and
held to tests/tree_cases.py's checker: C1 order, C2 vectors, C3 leaf boxes (bitwise the fused
form of the kernel's formula), C4 inner boxes, C5 soundness against the exact f64 values with
the derived slack bar, C6 the split every path guarantees (within its key's quantum), C7
adopters.  Each case asserts from L, G, H and the roles that the path it is named for was taken,
and both slots and both trees of the recorded pair are checked, with the inputs taken from the
setup record armed in the same call.

Shapes: the smallest that reach each path (tree.hpp: leaves of 64 points, level-G nodes of 4,096,
LDS partition above 512 points a sub-node, wave sorts of 512 / 256 / 128 keys, the multi-pass
levels below 32 (3-D) / 64 (12-D) builder nodes).
"""
import contextlib

import numpy as np
import pytest

import tree_cases as T

pytestmark = pytest.mark.gpu

LOW = dict(max_num_iterations=2, max_num_se3_iterations=1)
FRESH_SLOT = 0 | 9 << 8  # an engine slot no other test of the suite touches (0, 1, 2, 5, 6, 7, 11, 13 are taken)
TREES = ("src3", "tgt3", "src12", "tgt12")
ARRAYS = ("perm", "pos", "vec", "tvec", "tvec64", "tpt64", "lo", "hi")
SCALARS = ("n", "D", "L", "nnodes", "G", "H", "role", "written")


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
    """The five-scan chain of the sharing tests (~12,500 points a scan)."""
    return _scans(5, 200)


@pytest.fixture(scope="module")
def scans16():
    s = _scans(16, 135)
    assert all(8192 < x.shape[0] <= 16384 for x in s)
    return s


@pytest.fixture(scope="module")
def generic(bunny_unique):
    """Generic points (bunny vertices, shuffled) to cut clouds of exact sizes from."""
    rng = np.random.default_rng(3)
    return np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])], dtype=np.float64)


@pytest.fixture(scope="module")
def bunny_clouds(bunny_unique):
    """Four different clouds of 3,001 .. 3,544 points (test_gpu_tree_adopt.py's)."""
    from se3icp import datasets
    out = []
    for seed in (2, 3):
        src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=seed, subsample=0.1)
        out += [src, tgt]
    out[2] = out[2][:3001].copy()
    return [np.ascontiguousarray(c, dtype=np.float64) for c in out]


class DeviceBatch:
    """The pairs' clouds in two device buffers (sources, targets), every use a copy of its own."""

    def __init__(self, pairs):
        import torch
        self.src_off = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
        self.tgt_off = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
        src = np.ascontiguousarray(np.concatenate([s for s, _ in pairs]), dtype=np.float64)
        tgt = np.ascontiguousarray(np.concatenate([t for _, t in pairs]), dtype=np.float64)
        self.d_src, self.d_tgt = torch.from_numpy(src).to("cuda"), torch.from_numpy(tgt).to("cuda")
        torch.cuda.synchronize()

    def args(self):
        return self.d_src.data_ptr(), self.src_off, self.d_tgt.data_ptr(), self.tgt_off


@contextlib.contextmanager
def engine_modes(mod, sharing=0, tree=0, device=0):
    mod.set_batch_sharing(sharing, device)
    mod.set_tree_sharing(tree, device)
    try:
        yield
    finally:
        mod.set_batch_sharing(0, device)
        mod.set_tree_sharing(0, device)


def recorded(mod, p, ns, nt, n_max, call, device=0):
    """The tree record and the setup record of result slot p, armed together for the one call."""
    with mod.tree_record(p, ns, nt, device, n_max=n_max) as tr, mod.setup_record(p, ns, nt, device) as sr:
        res = call()
    return tr, sr, res


def record_batch(mod, pairs, p, method, prm, device=0):
    n_max = max(max(s.shape[0], t.shape[0]) for s, t in pairs)
    return recorded(mod, p, pairs[p][0].shape[0], pairs[p][1].shape[0], n_max,
                    lambda: mod.register_batch(pairs, method, prm, device), device)


def inputs_of(tr, sr, n_max):
    """Per tree of the record the checker's inputs, from the setup record of the same call."""
    out = {}
    for side, name in (("src", "src3"), ("tgt", "tgt3")):
        out[name] = T.inputs_3d(sr[side]["xyz"], sr[side]["f32_center"], n_max)
    for side, name in (("src", "src12"), ("tgt", "tgt12")):
        out[name] = None if sr[side]["rows"] is None else T.inputs_12d(sr[side]["rows"], n_max)
    return out


def check_record(name, tr, inputs, parity_record, trees=TREES, c6="quantised"):
    """check_tree on every tree of the record that the call builds (`trees`; the others must be
    absent); the `written` masks; the figures into the parity record.  Returns {tree: stats}."""
    stats, bad = {}, []
    for k in TREES:
        t = tr[k]
        if k not in trees:
            assert t is None, (name, k)
            continue
        assert t is not None, (name, k)
        side = 0 if k.startswith("src") else 1
        assert t["written"] == T.expected_written(t["D"], side, t["L"]), (name, k, t["written"])
        st = {}
        v = T.check_tree(t, inputs[k], st, c6=c6)
        stats[k] = st
        bad += [f"{name} {k}: {x}" for x in v]
        fig = {f"{k}.{a}": b for a, b in st.items() if a != "split_nodes"}
        fig.update({f"{k}.nodes.{path}": cnt for path, cnt in st.get("split_nodes", {}).items()})
        fig.update({f"{k}.L": t["L"], f"{k}.G": t["G"], f"{k}.H": t["H"], f"{k}.n": t["n"], f"{k}.role": t["role"]})
        parity_record(f"tree record: {name}", **fig)
        print(f"[tree record] {name} {k}: n {t['n']} L {t['L']} G {t['G']} H {t['H']} role {t['role']} {st}")
    assert not bad, bad
    for k, st in stats.items():
        if "slack_min_u" in st:
            assert st["slack_min_u"] >= 2.0, (name, k, st)  # (what C5 asserts per face, in the record's unit)
    return stats


def shape(tr, L, G, H3, H12=None, se3=True):
    """The depth and the levels of every tree of the record: the intended path was taken."""
    for k in TREES:
        if tr[k] is None:
            assert not se3 and k.endswith("12")
            continue
        want = (L, G, H12 if (k.endswith("12") and H12 is not None) else H3)
        assert (tr[k]["L"], tr[k]["G"], tr[k]["H"]) == want, (k, tr[k]["L"], tr[k]["G"], tr[k]["H"], want)


def paths(tr, k):
    return {T.level_path(tr[k], l) for l in range(tr[k]["L"])}


def as_bytes(tr):
    out = {}
    for k in TREES:
        if tr[k] is None:
            out[k] = None
            continue
        for a in ARRAYS:
            out[f"{k}.{a}"] = None if tr[k][a] is None else tr[k][a].tobytes()
        for a in SCALARS:
            out[f"{k}.{a}"] = tr[k][a]
    return out


# ------------------------------------------------------------------ 1. L = 0
@pytest.mark.parametrize("ns", [40, 1, 2])
def test_single_leaf(se3icp_mod, generic, parity_record, ns):
    """Clouds of at most 64 points: no level, k_tree_finish + k_tree_leafbox (+ k_tree_up over
    nothing).  At depth 0 the 12-D source tree is written like every other."""
    mod = se3icp_mod
    pairs = [(generic[100:100 + ns].copy(), generic[300:364].copy())]
    tr, sr, _ = record_batch(mod, pairs, 0, "se3_gicp", mod.default_params(number_of_nn_for_LRF=30, **LOW))
    shape(tr, 0, 0, 0)
    assert tr["src12"]["lo"] is not None and tr["src12"]["pos"] is not None
    assert (tr["src3"]["n"], tr["tgt3"]["n"], tr["tgt3"]["nnodes"]) == (ns, 64, 1)
    check_record(f"L0 {ns} onto 64", tr, inputs_of(tr, sr, 64), parity_record)


# ------------------------------------------------------------------ 2. local levels only
@pytest.mark.parametrize("ns,nt", [(65, 129), (2048, 2048), (4089, 4096), (4096, 4096)])
def test_local_levels(se3icp_mod, generic, parity_record, ns, nt):
    """G = 0: one workgroup per cloud (k_tree_local<D, false>) splits every level, writes the order,
    the vectors, the leaf boxes and the inner boxes; at 4,089 .. 4,096 points full leaves of 64,
    three LDS-partition levels and the sorts of 512, 256 and 128 keys."""
    mod = se3icp_mod
    pairs = [(generic[:ns].copy(), np.ascontiguousarray(generic[5000:5000 + nt] * 0.9 + 0.01))]
    tr, sr, _ = record_batch(mod, pairs, 0, "se3_gicp", mod.default_params(number_of_nn_for_LRF=30, **LOW))
    L = T.tree_depth_for(nt)
    shape(tr, L, 0, 0)
    if nt == 4096:
        assert L == 6 and paths(tr, "tgt3") == {"lds_partition", "sort512", "sort256", "sort128"}
        assert [T.level_path(tr["tgt12"], l) for l in range(6)] == ["lds_partition"] * 3 + ["sort512", "sort256", "sort128"]
    if nt == 129:
        assert L == 2 and paths(tr, "tgt3") == {"sort256", "sort128"}
    st = check_record(f"G0 {ns} onto {nt}", tr, inputs_of(tr, sr, nt), parity_record)
    assert tr["src12"]["lo"] is None and tr["src12"]["pos"] is None and tr["src12"]["tvec"] is None  # order only
    if ns == 4096:
        assert st["src3"]["empty_leaves"] == 0 and np.all(np.diff(T._leaf_ranges(4096, 6)) == 64)


# ------------------------------------------------------------------ 3. the multi-pass global levels
def test_multipass_one_level_beside_a_sparse_tree(se3icp_mod, generic, parity_record):
    """4,097 onto 40: one global level through k_tree_bbox / k_part_*; the 40-point target sits in a
    depth-7 tree whose leaves hold one point or none, so most boxes are [+inf, -inf], many inner
    nodes have an empty child, and its sub-nodes hold no sample point (the empty-sample fallback)."""
    mod = se3icp_mod
    pairs = [(generic[:4097].copy(), generic[6000:6040].copy())]
    tr, sr, _ = record_batch(mod, pairs, 0, "se3_gicp", mod.default_params(number_of_nn_for_LRF=30, **LOW))
    shape(tr, 7, 1, 1)
    assert T.level_path(tr["src3"], 0) == "multipass" and T.level_path(tr["src3"], 1) == "lds_partition"
    st = check_record("multipass 4097 onto 40", tr, inputs_of(tr, sr, 4097), parity_record)
    assert st["tgt3"]["empty_leaves"] == 88 and st["tgt12"]["empty_leaves"] == 88
    assert np.isinf(tr["tgt3"]["lo"]).any() and np.isfinite(tr["tgt3"]["lo"][0]).all()


def test_multipass_two_levels(se3icp_mod, scans5, parity_record):
    """8,193 onto 16,384: G = 2, both global levels multi-pass (two builders: 2 and 4 nodes)."""
    mod = se3icp_mod
    big = np.ascontiguousarray(np.concatenate([scans5[0], scans5[1]])[:16384])
    pairs = [(scans5[2][:8193].copy(), big)]
    tr, sr, _ = record_batch(mod, pairs, 0, "se3_gicp", mod.kitti_params(**LOW))
    shape(tr, 8, 2, 2)
    check_record("multipass 8193 onto 16384", tr, inputs_of(tr, sr, 16384), parity_record)


# ------------------------------------------------------------------ 4. k_tree_level
def _ring16(scans16):
    return [(scans16[(i + 1) % 16], scans16[i]) for i in range(16)]


def test_level_kernel(se3icp_mod, scans16, parity_record):
    """Sixteen pairs of ~8.4k-point scans, a host batch (32 builders): the 3-D build has 32 nodes at
    level 0 already, so H = 0 < G = 2 and both global levels are k_tree_level launches; the 12-D
    build (64 nodes wanted) takes the multi-pass sequence at level 0 and k_tree_level at level 1 --
    this size reaches k_tree_level for both trees."""
    mod = se3icp_mod
    pairs = _ring16(scans16)
    n_max = max(s.shape[0] for s in scans16)
    for p in (0, 15):
        tr, sr, _ = record_batch(mod, pairs, p, "se3_gicp", mod.kitti_params(**LOW))
        shape(tr, 8, 2, 0, H12=1)
        assert tr["src3"]["H"] < tr["src3"]["G"] and tr["tgt12"]["H"] < tr["tgt12"]["G"]
        assert [T.level_path(tr["tgt3"], l) for l in (0, 1)] == ["k_tree_level"] * 2
        assert [T.level_path(tr["tgt12"], l) for l in (0, 1)] == ["multipass", "k_tree_level"]
        assert mod.last_tree_stats() == {"built_3d": 32, "adopted_3d": 0, "built_12d": 32, "adopted_12d": 0}
        check_record(f"level kernel pair {p}", tr, inputs_of(tr, sr, n_max), parity_record)


# ------------------------------------------------------------------ 5. adoption
def _check_adopters(name, recs, n_max, parity_record, expect_adopters):
    """recs: per pair (tree record, setup record).  Every tree through the checker; every adopter
    against its donor's record (C7), its tree-ordered vectors and boxes differing from the donor's
    where the pair scale does -- at one adopter at least in every case that has adopters (a scan
    that holds the farthest point of both its pairs has one scale in both: scan 1 of the chain)."""
    adopters = {3: [], 12: []}
    differing = 0
    for p, (tr, sr) in enumerate(recs):
        check_record(f"{name} pair {p}", tr, inputs_of(tr, sr, n_max), parity_record)
        for k in TREES:
            t = tr[k]
            if t["role"] < 0:
                continue
            donor = recs[t["role"] // 2][0][("src" if t["role"] % 2 == 0 else "tgt") + k[3:]]
            assert donor["role"] == T.BUILT
            slot = 2 * p + (0 if k.startswith("src") else 1)
            adopters[t["D"]].append(slot)
            assert T.check_adopter(t, donor) == [], (name, p, k)
            own = sr["src" if k.startswith("src") else "tgt"]["norm_scale"]
            don = recs[t["role"] // 2][1]["src" if t["role"] % 2 == 0 else "tgt"]["norm_scale"]
            if t["D"] == 3 and own != don:  # (both 3-D trees have boxes; a 12-D source donor is order only)
                differing += 1
                assert T.boxes_differ(t, donor), (name, p, k)
                assert t["tvec"].tobytes() != donor["tvec"].tobytes(), (name, p, k)
            if t["D"] == 12 and t["lo"] is not None and donor["lo"] is not None and own != don:
                assert T.boxes_differ(t, donor), (name, p, k)
    assert adopters[3] == expect_adopters and adopters[12] == expect_adopters, (name, adopters)
    assert differing >= 1 or not expect_adopters, (name, differing)


def _stats(built, adopted):
    return {"built_3d": built, "adopted_3d": adopted, "built_12d": built, "adopted_12d": adopted}


@pytest.mark.parametrize("sharing,tree", [(2, 0), (2, 1), (1, 0)])
def test_chain_graph(se3icp_mod, scans5, parity_record, sharing, tree):
    """register_graph over the five-scan chain: scans 1, 2 and 3 lie in two slots each under two
    scales; with tree sharing the second slot adopts the first one's order (k_tree_local<D, true>)
    and must have its OWN vectors and boxes."""
    mod = se3icp_mod
    edges = mod.sequence_edges(5)
    pairs = mod.expand_edges(scans5, edges)
    n_max = max(s.shape[0] for s in scans5)
    prm = mod.kitti_params(**LOW)
    adopt = sharing >= 2 and tree == 0
    recs = []
    for p in range(4):
        with engine_modes(mod, tree=tree):
            tr, sr, _ = recorded(mod, p, pairs[p][0].shape[0], pairs[p][1].shape[0], n_max,
                                 lambda: mod.register_graph(scans5, edges, "se3_gicp", prm, sharing=sharing))
            assert mod.last_tree_stats() == (_stats(5, 3) if adopt else _stats(8, 0))
        # five builders (eight without sharing): 5, 10 / 8, 16 nodes, both global levels multi-pass
        shape(tr, 8, 2, 2)
        recs.append((tr, sr))
    _check_adopters(f"chain graph sharing {sharing} tree {tree}", recs, n_max, parity_record, [3, 5, 7] if adopt else [])


@pytest.mark.parametrize("sharing,tree", [(2, 0), (2, 1), (1, 0)])
def test_chain_reversed_device_batch(se3icp_mod, scans5, parity_record, sharing, tree):
    """The chain as a device batch in reverse order (slots s4 s3 | s3 s2 | s2 s1 | s1 s0): the
    donors build behind the compare flags' first build, the adopters in the second."""
    mod = se3icp_mod
    pairs = mod.expand_edges(scans5, mod.sequence_edges(5))[::-1]
    n_max = max(s.shape[0] for s in scans5)
    prm = mod.kitti_params(**LOW)
    batch = DeviceBatch(pairs)
    adopt = sharing == 2 and tree == 0
    recs = []
    for p in range(4):
        with engine_modes(mod, sharing=sharing, tree=tree):
            tr, sr, _ = recorded(mod, p, pairs[p][0].shape[0], pairs[p][1].shape[0], n_max,
                                 lambda: mod.register_batch_device(*batch.args(), "se3_gicp", prm))
            assert mod.last_tree_stats() == (_stats(5, 3) if adopt else _stats(8, 0))
        recs.append((tr, sr))
    _check_adopters(f"chain device sharing {sharing} tree {tree}", recs, n_max, parity_record, [2, 4, 6] if adopt else [])


def test_bunny_adopters_without_a_global_level(se3icp_mod, bunny_clouds, parity_record):
    """Four clouds of ~3k points (G = 0), cloud 1 in five slots: four adopters of one donor."""
    mod = se3icp_mod
    pairs = mod.expand_edges(bunny_clouds, [(1, 0), (2, 1), (3, 1), (1, 1)])
    n_max = max(c.shape[0] for c in bunny_clouds)
    prm = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    batch = DeviceBatch(pairs)
    recs = []
    for p in range(4):
        tr, sr, _ = recorded(mod, p, pairs[p][0].shape[0], pairs[p][1].shape[0], n_max,
                             lambda: mod.register_batch_device(*batch.args(), "se3_gicp", prm))
        assert mod.last_tree_stats() == _stats(4, 4)
        shape(tr, 6, 0, 0)
        recs.append((tr, sr))
    _check_adopters("bunny adopters", recs, n_max, parity_record, [3, 5, 6, 7])


# ------------------------------------------------------------------ 6. the raw frame
def test_raw_frame_at_utm_offsets(se3icp_mod, scans5, parity_record):
    """gicp (run_icp): no normalization, the clouds at (4.5e5, 5.4e6, 300); the f32 vectors are
    float32(xyz - f32_center) about the target's centre and the boxes bound the exact shifted
    values; no 12-D tree exists."""
    mod = se3icp_mod
    off = np.array([4.5e5, 5.4e6, 300.0])
    pairs = [(np.ascontiguousarray(scans5[1][:4097] + off), np.ascontiguousarray(scans5[0][:6145] + off))]
    tr, sr, _ = record_batch(mod, pairs, 0, "gicp", mod.kitti_params(**LOW))
    assert tr["src12"] is None and tr["tgt12"] is None
    for side in ("src", "tgt"):
        assert np.abs(sr[side]["f32_center"] - off).max() < 100 and sr[side]["norm_scale"] == 1.0
        assert sr[side]["xyz"].tobytes() == pairs[0][0 if side == "src" else 1].tobytes()
    shape(tr, 7, 1, 1, se3=False)
    st = check_record("raw frame gicp", tr, inputs_of(tr, sr, 6145), parity_record, trees=("src3", "tgt3"))
    # the shift matters: about the origin the f32 grid at 5.4e6 is 0.5 wide
    assert np.abs(tr["tgt3"]["vec"]).max() < 1000.0 and st["tgt3"]["slack_min_u"] >= 2.0


# ------------------------------------------------------------------ 7. designed vectors
def _nn_record(mod, query, data, device=0):
    n_max = max(len(query), len(data))
    with mod.tree_record(0, len(query), len(data), device, n_max=n_max) as tr:
        idx, _, _ = mod.nearest_neighbors(query, data, device=device)
    assert ((idx >= 0) & (idx < len(data))).all()
    return tr, n_max


def _bare_boxes(t):
    """The tree with the uninflated f32 extremes for boxes (the 'no inflation' defect)."""
    vlo, vhi = T._leaf_extremes(t["tvec"], t["n"], t["L"])
    lo, hi = T._fold(vlo, vhi, t["L"])
    return dict(t, lo=lo, hi=hi)


@pytest.mark.parametrize("n", [200, 4097])
@pytest.mark.parametrize("kind", T.KINDS)
def test_designed_3d(se3icp_mod, parity_record, kind, n):
    """Designed 3-D vectors straight into the build (se3icp_nn): the queries carry them as they
    are, the data is (p, -p) interleaved, whose centre is exactly 0, so float32(x - centre) is
    float32(x) for both and the designed values reach the boxes."""
    mod = se3icp_mod
    q = T.designed(kind, n, 3)
    data = T.symmetric(T.designed(kind, (n + 1) // 2, 3, seed=1))[:n]
    if n % 2:
        data = np.ascontiguousarray(np.concatenate([data[:-1], np.zeros((1, 3))]))
    cen = T.nn_center(data)
    assert not cen.any()
    tr, n_max = _nn_record(mod, q, data)
    assert tr["src12"] is None and tr["tgt12"] is None
    inputs = {"src3": T.inputs_3d(q, cen, n_max), "tgt3": T.inputs_3d(data, cen, n_max)}
    shape(tr, T.tree_depth_for(n), 1 if n > 4096 else 0, 1 if n > 4096 else 0, se3=False)
    st = check_record(f"designed 3-D {kind} {n}", tr, inputs, parity_record, trees=("src3", "tgt3"))
    _designed_figures(kind, tr, inputs, st, "src3")


@pytest.mark.parametrize("n", [200, 4097])
@pytest.mark.parametrize("kind", T.KINDS)
def test_designed_12d(se3icp_mod, parity_record, kind, n):
    """Designed 12-D vectors: the data's tree has the boxes (the queries' is order only)."""
    mod = se3icp_mod
    q, data = T.designed(kind, n, 12), T.designed(kind, n, 12, seed=1)
    tr, n_max = _nn_record(mod, q, data)
    inputs = {"src12": T.inputs_12d(q, n_max), "tgt12": T.inputs_12d(data, n_max)}
    G = 1 if n > 4096 else 0
    for k in ("src12", "tgt12"):
        assert (tr[k]["L"], tr[k]["G"], tr[k]["H"]) == (T.tree_depth_for(n), G, G), k
    stats = check_record(f"designed 12-D {kind} {n}", tr, inputs, parity_record, trees=("src12", "tgt12"))
    assert tr["src12"]["lo"] is None and tr["src12"]["tvec"] is None and tr["src12"]["pos"] is None
    _designed_figures(kind, tr, inputs, stats, "tgt12")


def _designed_figures(kind, tr, inputs, st, k):
    f32 = np.float32
    t = tr[k]
    if kind == "zero":
        assert (t["lo"][:, 2] == -f32(1e-30)).all() and (t["hi"][:, 2] == f32(1e-30)).all()
    if kind == "negative" and k == "src3":
        assert (t["hi"] < 0).all()
    if kind == "tworound":
        assert st[k]["fused_differs"] > 0  # (the two-rounding form would have written other bits, and C3 passed)
        assert any(x.startswith("C3") for x in T.check_tree(t, inputs[k], box=T.box_two_roundings, c6="quantised"))
    if kind == "outward":
        v = T.check_tree(_bare_boxes(t), inputs[k], c6="quantised")
        assert any(x.startswith("C5 containment") for x in v), v
    if kind == "copies":
        assert (t["lo"][(1 << t["L"]) - 1:] < t["hi"][(1 << t["L"]) - 1:]).all()  # (inflated: never zero extent)


def test_sweep_second_group(se3icp_mod, generic, parity_record):
    """register_sweep, three variants in groups of two: variant 2 is in the second group, whose 3-D
    trees are k_sweep_expand's copies of the shared setup's and whose 12-D trees are its own."""
    mod = se3icp_mod
    pairs = [(generic[:40].copy(), generic[7000:10001].copy()), (generic[:6145].copy(), generic[10000:14097].copy())]
    base = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    variants = mod.sweep_params(base, alpha_rot=[1.0, 0.5, 3.0], beta_transl=[1.0, 2.0, 0.7])
    n_max = 6145
    seen = {}
    for v, p in ((2, 0), (2, 1), (1, 0), (1, 1)):  # variant 1: replica 1 of the first group (offsets k N)
        tr, sr, _ = recorded(mod, v * 2 + p, pairs[p][0].shape[0], pairs[p][1].shape[0], n_max,
                             lambda: mod.register_sweep(pairs, "se3_gicp", variants, max_group=2))
        assert (sr["src"]["alpha"], sr["src"]["beta"]) == (variants[v].alpha_rot, variants[v].beta_transl)
        shape(tr, 7, 1, 1)
        check_record(f"sweep variant {v} pair {p}", tr, inputs_of(tr, sr, n_max), parity_record)
        seen[(v, p)] = as_bytes(tr)
    for p in (0, 1):  # a replica's 3-D trees are copies of its base cloud's, whatever the variant
        a, b = seen[(1, p)], seen[(2, p)]
        assert not [k for k in a if k.split(".")[0] in ("src3", "tgt3") and a[k] != b[k]]
        assert a["tgt12.lo"] != b["tgt12.lo"]  # (the 12-D rows carry the variant's weights)


# ------------------------------------------------------------------ 8. determinism, arming
def test_deterministic_on_a_fresh_engine(se3icp_mod, generic, scans16, parity_record):
    """The sparse multi-pass case and the sixteen-pair case twice each on an engine slot no other
    test touches (its first calls): the whole record is bitwise equal, and equal to slot 0's."""
    mod = se3icp_mod
    cases = [("4097 onto 40", [(generic[:4097].copy(), generic[6000:6040].copy())], 0,
              mod.default_params(number_of_nn_for_LRF=30, **LOW)),
             ("16 pairs", _ring16(scans16), 15, mod.kitti_params(**LOW))]
    for name, pairs, p, prm in cases:
        a = as_bytes(record_batch(mod, pairs, p, "se3_gicp", prm, device=FRESH_SLOT)[0])
        b = as_bytes(record_batch(mod, pairs, p, "se3_gicp", prm, device=FRESH_SLOT)[0])
        c = as_bytes(record_batch(mod, pairs, p, "se3_gicp", prm)[0])
        diff = [k for k in a if a[k] != b[k] or a[k] != c[k]]
        parity_record(f"tree record: determinism {name}", equal=not diff)
        assert not diff, (name, diff)


def test_arming_rules(se3icp_mod, generic):
    """One-shot; a pair outside the call's results and arrays too small for the tree are
    SE3ICP_ERR_INVALID_ARG from that call, before its loop; unarmed and armed calls return the
    same bits; se3icp_nn accepts pair 0 only."""
    import ctypes as C
    from se3icp import _lib
    mod = se3icp_mod
    pairs = [(generic[:40].copy(), generic[7000:10001].copy())]
    prm = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    want = mod.register_batch(pairs, "se3_gicp", prm)
    with pytest.raises(_lib.Se3IcpError) as e:
        with mod.tree_record(1, 40, 3001):
            mod.register_batch(pairs, "se3_gicp", prm)
    assert e.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.Se3IcpError) as e:
        with mod.tree_record(0, 40, 3000, n_max=3001):  # the target's arrays one point short
            mod.register_batch(pairs, "se3_gicp", prm)
    assert e.value.code == _lib.ERR_INVALID_ARG
    rec = _lib.TreeRecord()  # room for 126 nodes where the trees have 127
    box = np.zeros((126, 3), np.float32)
    rec.tgt3.lo = box.ctypes.data_as(C.POINTER(C.c_float))
    rec.tgt3.node_cap = 126
    _lib.check(_lib.load().se3icp_set_tree_record(0, C.byref(rec)))
    with pytest.raises(_lib.Se3IcpError) as e:
        mod.register_batch(pairs, "se3_gicp", prm)
    assert e.value.code == _lib.ERR_INVALID_ARG and rec.recorded == 0 and not box.any()
    rec = _lib.TreeRecord()  # no arrays: the scalars alone
    _lib.check(_lib.load().se3icp_set_tree_record(0, C.byref(rec)))
    got = mod.register_batch(pairs, "se3_gicp", prm)
    assert rec.recorded == 1 and (rec.src3.n, rec.tgt12.n, rec.tgt3.L, rec.tgt3.nnodes) == (40, 3001, 6, 127)
    assert rec.src3.written == 0 and rec.tgt12.exists == 1 and rec.tgt3.role == _lib.TREE_BUILT
    rec.recorded = 0
    again = mod.register_batch(pairs, "se3_gicp", prm)  # disarmed by the call before
    assert rec.recorded == 0
    for r in (got, again):
        assert r[0].T.tobytes() == want[0].T.tobytes() and r[0].num_iterations == want[0].num_iterations
    with pytest.raises(_lib.Se3IcpError) as e:
        with mod.tree_record(1, 10, 10):
            mod.nearest_neighbors(generic[:10], generic[10:20])
    assert e.value.code == _lib.ERR_INVALID_ARG
