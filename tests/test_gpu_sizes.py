"""GPU parity at the sizes that fill a tree structure exactly.

The other GPU tests run at the fixture (4,167 points), the bunny (35k), RGB-D frames and
120k-point scans, where leaves hold 32-59 points (never kLeafMax = 64), an NN work chunk at
most 938 positions (never kChunkQ = 1024) and a workgroup-local node of k_tree_local about
3,750 points (never kLocalMax = 4096).  This file runs the stage entry points against the
oracle at cloud sizes n around the powers of two:

* outside the window: n = 1, 2, 63 .. 65 (one leaf / two), 128 .. 2049 (leaves of exactly 64
  and, at 2048, a chunk of exactly 1024 and wave sorts of exactly 128 / 256 / 512 keys),
  4088 / 4097 and 8176 / 8193 (the sizes next to the window);
* inside the window (tests named test_window_*): ceil(n / 2^G) in 4089 .. 4096, where the
  level-G nodes hold kLocalMax points.  There k_tree_local sent eight sub-nodes of 512 points
  through its LDS partition (laid out for four) and zeroed the node's permutation, and a
  se3icp_nn call that was an engine's first read a setup table that did not exist
  (tests/test_tree_layout.py checks the arithmetic for every n on the CPU).

Data are drawn from continuous distributions (no exact ties; the 12-D rows are
alpha-weighted rotations plus translations as in test_adversarial_near_ties_at_120k), so
indices must equal the oracle's and d2 agree to 1e-12 (test_nn_few_queries_against_large_data's
bars).  se3icp_nn takes the tree depth from max(nq, nd), so a size is exercised only with
nq = nd = n; each NN case is therefore two calls of n queries: the data rows themselves
(every target must be found by its own copy at d2 = 0: a point lost from the permutation
fails) and n random rows (against the oracle).  Stage outputs (kNN, TOLDI frames, normals)
are compared under test_gpu_parity's rules, tolerances unchanged.
"""
import numpy as np
import pytest

from test_gpu_parity import _eig_gap, _toldi_cov
from test_gpu_trace import _near_tie_queries

pytestmark = pytest.mark.gpu

NN_SIZES = [1, 2, 63, 64, 65, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4088, 4097, 8176, 8193]
NN_LOPSIDED = [(2048, 70), (70, 2048)]
STAGE_SIZES = [64, 65, 2048, 4088, 4097]
WINDOW_NN_SIZES = [4089, 4096, 8177, 8192, 16384]
FRESH_SLOT = 11  # an engine slot no other test of the suite touches (test_gpu_parity: 0, 1, 2)
K = 30


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


@pytest.fixture(scope="module")
def refcpu():
    from oracle import refcpu as r
    r.lib()
    return r


def _rows(dim, n, rng):
    if dim == 12:  # SE(3)-element-like vectors: alpha-weighted rotations + translations
        from scipy.spatial.transform import Rotation
        R = Rotation.random(n, random_state=int(rng.integers(1 << 31))).as_matrix().reshape(n, 3, 3)
        t = rng.uniform(-3, 3, (n, 3))
        return np.ascontiguousarray(np.concatenate([3.0 * R.transpose(0, 2, 1).reshape(n, 9), t], axis=1))
    return rng.uniform(-3, 3, (n, 3))


def _nn_case(se3icp_mod, refcpu, dim, n, device=0):
    """Both calls of one size (see the module docstring); returns the rechecked counts."""
    rng = np.random.default_rng(1000 * dim + n)
    data = _rows(dim, n, rng)
    gi, gd2, r0 = se3icp_mod.nearest_neighbors(data, data, device=device)
    assert np.array_equal(gi, np.arange(n)), (dim, n, "own copy", np.nonzero(gi != np.arange(n))[0][:8])
    assert not gd2.any(), (dim, n, gd2.max())
    q = _rows(dim, n, rng)
    gi, gd2, r1 = se3icp_mod.nearest_neighbors(q, data, device=device)
    ri, rd2 = refcpu.nn(q, data)
    assert np.array_equal(gi, ri), (dim, n, np.nonzero(gi != ri)[0][:8])
    np.testing.assert_allclose(gd2, rd2, rtol=0, atol=1e-12)
    return r0, r1


# --------------------------------------------------------------------------- outside the window
@pytest.mark.parametrize("dim", [3, 12])
@pytest.mark.parametrize("n", NN_SIZES)
def test_nn_at_structural_sizes(se3icp_mod, refcpu, dim, n, parity_record):
    r0, r1 = _nn_case(se3icp_mod, refcpu, dim, n)
    parity_record(f"sizes: nn {dim}-D n={n}", rechecked_own_copies=r0, rechecked_random=r1)


@pytest.mark.parametrize("dim", [3, 12])
@pytest.mark.parametrize("nq,nd", NN_LOPSIDED)
def test_nn_lopsided_pairs(se3icp_mod, refcpu, dim, nq, nd):
    """One cloud fills leaves and a chunk exactly, the other shares its depth with 1-3
    points per leaf.  Half the queries (at most nd) are copies of data rows."""
    rng = np.random.default_rng(7000 + 10 * dim + nq)
    data = _rows(dim, nd, rng)
    own = np.sort(rng.choice(nd, min(nq // 2, nd), replace=False))
    q = np.ascontiguousarray(np.concatenate([data[own], _rows(dim, nq - own.size, rng)]))
    gi, gd2, _ = se3icp_mod.nearest_neighbors(q, data)
    ri, rd2 = refcpu.nn(q, data)
    assert np.array_equal(gi[:own.size], own) and not gd2[:own.size].any()
    assert np.array_equal(gi, ri), np.nonzero(gi != ri)[0][:8]
    np.testing.assert_allclose(gd2, rd2, rtol=0, atol=1e-12)


_STAGE_REF = {}


def _stage_ref(refcpu, n):
    """The cloud of a stage size and its oracle outputs, computed once and left unchanged."""
    if n not in _STAGE_REF:
        pts = np.random.default_rng(3000 + n).uniform(-3, 3, (n, 3))
        idx, d2 = refcpu.knn_self(pts, K)
        ref = {"pts": pts, "knn_idx": idx, "knn_d2": d2, "frames": refcpu.toldi_frames(pts, K),
               "normals": refcpu.estimate_normals(pts, K)}
        for v in ref.values():
            v.setflags(write=False)
        _STAGE_REF[n] = ref
    return _STAGE_REF[n]


def _check_knn(g, ref):
    """test_knn_self_matches_oracle's rule."""
    pts, ri, rd = ref["pts"], ref["knn_idx"], ref["knn_d2"]
    same = (g == ri)
    for i in np.nonzero(~same.all(axis=1))[0]:  # allowed only where the lists differ by exact-distance ties
        dg = np.sum((pts[g[i]] - pts[i]) ** 2, axis=1)
        np.testing.assert_allclose(np.sort(dg), rd[i], rtol=0, atol=1e-12)
    d = np.sum((pts[g] - pts[:, None, :]) ** 2, axis=2)
    assert (np.diff(d, axis=1) >= -1e-15).all()
    assert (g >= 0).all() and (g < len(pts)).all()
    return int((~same.all(axis=1)).sum())


def _check_frames(g, ref):
    """test_toldi_frames_match_oracle's rule."""
    pts, r, idx = ref["pts"], ref["frames"], ref["knn_idx"]
    diff = np.abs(g - r).reshape(len(pts), -1).max(axis=1)
    bad = np.nonzero(diff > 1e-8)[0]
    assert len(bad) <= 0.001 * len(pts), np.sort(diff)[-10:]
    if len(bad):
        gap = _eig_gap(_toldi_cov(pts, idx[bad]))
        z = r[bad, :3, 2]
        v = pts[idx[bad, 1:]] - pts[bad, None, :]
        R = np.linalg.norm(pts[idx[bad, -1]] - pts[bad], axis=1)
        w = (R[:, None] - np.linalg.norm(v, axis=2)) ** 2 * np.einsum("nki,ni->nk", v, z) ** 2
        acc = np.einsum("nk,nki->ni", w, v)
        xr = np.linalg.norm(acc - np.einsum("ni,ni->n", acc, z)[:, None] * z, axis=1)
        xr = xr / np.maximum(np.linalg.norm(acc, axis=1), 1e-300)
        ill = (gap < 1e-6) | (xr < 1e-6)
        assert ill.all(), (bad[~ill], diff[bad[~ill]], gap[~ill], xr[~ill])
    Rg = g[:, :3, :3]
    np.testing.assert_allclose(np.einsum("nij,nik->njk", Rg, Rg), np.broadcast_to(np.eye(3), Rg.shape), atol=1e-9)
    return len(bad), float(np.max(diff[diff <= 1e-8], initial=0.0))


def _check_normals(g, ref):
    """test_estimate_normals_match_oracle's rule."""
    pts, r, idx = ref["pts"], ref["normals"], ref["knn_idx"]
    diff = np.abs(g - r).max(axis=1)
    bad = np.nonzero(diff > 1e-8)[0]
    assert len(bad) <= 0.001 * len(pts)
    if len(bad):
        p = pts[idx[bad]]
        mu = p.mean(axis=1)
        cov = np.einsum("nki,nkj->nij", p, p) / K - np.einsum("ni,nj->nij", mu, mu)
        gap = _eig_gap(cov)
        assert (gap < 1e-6).all(), (bad[gap >= 1e-6], diff[bad[gap >= 1e-6]], gap[gap >= 1e-6])
    return len(bad), float(np.max(diff[diff <= 1e-8], initial=0.0))


@pytest.mark.parametrize("n", STAGE_SIZES)
def test_knn_frames_normals_at_structural_sizes(se3icp_mod, refcpu, n, parity_record):
    ref = _stage_ref(refcpu, n)
    pts = ref["pts"]
    ties = _check_knn(se3icp_mod.knn_self(pts, K), ref)
    fbad, fmax = _check_frames(se3icp_mod.toldi_frames(pts, K), ref)
    nbad, nmax = _check_normals(se3icp_mod.estimate_normals(pts, K), ref)
    parity_record(f"sizes: stages n={n} k={K}", lists_differing_in_tie_order=ties, frames_over_1e8=fbad,
                  frames_max_diff_well_conditioned=fmax, normals_over_1e8=nbad, normals_max_diff_well_conditioned=nmax)


# --------------------------------------------------------------------------- inside the window
@pytest.mark.parametrize("dim", [3, 12])
@pytest.mark.parametrize("n", WINDOW_NN_SIZES)
def test_window_nn(se3icp_mod, refcpu, dim, n, parity_record):
    r0, r1 = _nn_case(se3icp_mod, refcpu, dim, n)
    parity_record(f"sizes: window nn {dim}-D n={n}", rechecked_own_copies=r0, rechecked_random=r1)


def test_window_nn_32_full_local_nodes(se3icp_mod, refcpu, parity_record):
    """nd = 131,072 (an ordinary LiDAR scan size): five global levels, then 32 workgroups of
    k_tree_local with a node of exactly 4096 points each.  2,048 queries: 1,024 copies of
    data rows spread over the cloud and 1,024 random rows."""
    rng = np.random.default_rng(131072)
    nd, nq = 131072, 2048
    data = _rows(3, nd, rng)
    own = np.sort(rng.choice(nd, nq // 2, replace=False))
    q = np.ascontiguousarray(np.concatenate([data[own], _rows(3, nq - own.size, rng)]))
    gi, gd2, nrech = se3icp_mod.nearest_neighbors(q, data)
    ri, rd2 = refcpu.nn(q, data)
    parity_record("sizes: window nn 3-D nd=131072 nq=2048", rechecked=nrech)
    assert np.array_equal(gi[:own.size], own) and not gd2[:own.size].any()
    assert np.array_equal(gi, ri), np.nonzero(gi != ri)[0][:8]
    np.testing.assert_allclose(gd2, rd2, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dim", [12, 3])
def test_window_near_ties_at_8192(se3icp_mod, refcpu, dim, parity_record):
    """test_adversarial_near_ties_at_120k's queries at 8192 x 8192: full leaves, full chunks
    and full local nodes under the f64 recheck, whose answer must be the oracle's bit for bit."""
    rng = np.random.default_rng(8192 + dim)
    n = 8192
    data = _rows(dim, n, rng)
    q = _near_tie_queries(data, rng, n)
    gi, gd2, nrech = se3icp_mod.nearest_neighbors(q, data)
    ri, rd2 = refcpu.nn(q, data)
    mism = np.nonzero(gi != ri)[0]
    parity_record(f"sizes: window near-ties {dim}-D n=8192", queries=n, rechecked_f64=int(nrech),
                  index_differences=int(mism.size), d2_bit_differences=int((gd2 != rd2).sum()))
    assert mism.size == 0, (mism[:8], gi[mism[:8]], ri[mism[:8]])
    assert np.array_equal(gd2, rd2)


def test_window_knn_and_frames_at_4096_in_every_lrf_mode(se3icp_mod, refcpu, parity_record):
    """One full local node in the 3-D tree of the setup: the kNN lists and TOLDI frames of
    the default kernels, the exact kernel and the global-buffer kernel equal the oracle's and
    one another bit for bit."""
    from se3icp import registration
    ref = _stage_ref(refcpu, 4096)
    pts = ref["pts"]
    knn, frames = [], []
    try:
        for mode in (0, 1, 2):
            registration.set_lrf_exact(mode)
            knn.append(se3icp_mod.knn_self(pts, K))
            frames.append(se3icp_mod.toldi_frames(pts, K))
    finally:
        registration.set_lrf_exact(0)
    ties = _check_knn(knn[0], ref)
    fbad, fmax = _check_frames(frames[0], ref)
    parity_record(f"sizes: window stages n=4096 k={K}", lists_differing_in_tie_order=ties, frames_over_1e8=fbad,
                  frames_max_diff_well_conditioned=fmax)
    for mode in (1, 2):
        assert np.array_equal(knn[mode], knn[0]), mode
        assert np.array_equal(frames[mode].view(np.uint64), frames[0].view(np.uint64)), mode


@pytest.fixture(scope="module")
def pair_4096(bunny_unique):
    """4096 x 4096 points of datasets.bunny_pair(seed=2, subsample=0.125) (4398 / 4445 noisy
    points, a sorted random choice of each).  The oracle alone has no rounding-level near-tie
    in any iteration of either method below (0 candidates by test_gpu_params'
    _near_tie_candidates), so idx_diff == 0 excuses nothing."""
    from se3icp import datasets
    src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=2, subsample=0.125)
    assert (src.shape[0], tgt.shape[0]) == (4398, 4445)
    rng = np.random.default_rng(4096)
    src = src[np.sort(rng.choice(len(src), 4096, replace=False))]
    tgt = tgt[np.sort(rng.choice(len(tgt), 4096, replace=False))]
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt)


@pytest.mark.parametrize("variant", ["pt2pt", "gicp"])
def test_window_registration_4096_traced_and_untraced(se3icp_mod, refcpu, pair_4096, variant, parity_record):
    """The whole loop on clouds of exactly kLocalMax points (3-D and 12-D trees of both
    clouds with one full local node): iteration counts, idx_diff == 0 at every iteration,
    and the untraced run bitwise equal (test_gpu_params._traced_case)."""
    from test_gpu_params import B_BASE, _near_tie_candidates, _traced_case
    g, gtr, ref, tot = _traced_case(se3icp_mod, refcpu, parity_record, f"sizes: window 4096 se3_{variant}", pair_4096,
                                    "se3_" + variant, refcpu.RUN_SE3_ICP, variant, dict(B_BASE))
    assert _near_tie_candidates(ref) == 0


def test_window_first_call_on_a_fresh_engine_slot(se3icp_mod, refcpu):
    """A 12-D se3icp_nn as the first call an engine ever serves: k_nn_prep reads the source
    cloud's setup record, which only a registration used to allocate."""
    rng = np.random.default_rng(12)
    data = _rows(12, 300, rng)
    q = _rows(12, 200, rng)
    gi, gd2, _ = se3icp_mod.nearest_neighbors(q, data, device=FRESH_SLOT << 8)
    ri, rd2 = refcpu.nn(q, data)
    assert np.array_equal(gi, ri)
    np.testing.assert_allclose(gd2, rd2, rtol=0, atol=1e-12)
