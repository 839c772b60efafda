"""The setup stage on the GPU (the kNN lists, the TOLDI frames and the normals of k_knn.hip's
k_lrf, k_lrf8.hip and k_knn_big.hip, and the two eigen-solvers of devmath.hpp they share) against
the long-double restatement of lrf_reference.py, on the designed clouds and k values of its CASES.

Every point is held to conditioned measures (lrf_reference.py): the error of the z axis, the x
axis and the normal in units of the first-order rounding error of their own sums,

    K_z <= 8 KZ_ORACLE,   K_x <= 8 KX_ORACLE,   K_n <= 8 KN_ORACLE,

where the *_ORACLE are the largest values the oracle (f64, sequential sums) reaches on the same
cases in the same run (test_lrf_reference.py asserts they are of order one).  The kernels differ
from the oracle by eight strided partial sums and a butterfly instead of a sequential sum, the
moment expansion M - S cl^T - cl S^T + rz cl cl^T instead of per-point differences, and device
contraction: a small factor on the error constant.  A wrong rank range, divisor, radius or
weight is more than three orders above these bars (test_lrf_reference.py's power test).  The
designed clouds have no ill-conditioned point (its design conditions), so no point is left out.

Besides the measures: every output finite, |y - z x x|_inf <= 4 eps, the translation column
equal to the point bit for bit (the stage entries run with alpha = beta = 1), the z axis on the
side of the neighbours' sum, and knn_self equal to the brute-force lists (no ties here).

The k lists put rz = k // 3, rz - 1 and k - 1 on each side of multiples of 8 (the stride of the
sums passes), k mod 3 at every residue, and k on both sides of 128, where k_knn_big takes over;
the kinds add a partial last wave (517), the box path over more than 64 leaves (4,099) and
k > n (20 and 7 points).  Each case runs in the default mode and with every point through the
exact kernel (set_lrf_exact).

The exact cases reach the solver branches no scan reaches: a diagonal covariance (nrm == 0), the
zero covariance (mc == 0), fewer than three neighbours, and an exact plane.  Their coordinates
are multiples of 2^-4 below 8, so every cumulant sum is exact in any order and the normals are
asserted bit for bit, against the stated value and against the oracle.

Not asserted: frames on the exact plane (z . v is zero to rounding and the reference normalises
a zero x axis without a guard) and on the symmetric sets (their distance ties leave the rank
ranges to the search order), and k < 9 (rz <= 2: the reference's own frame is undefined).
"""
import contextlib

import numpy as np
import pytest

import lrf_reference as L
from lrf_reference import BAR_FACTOR, EPS

pytestmark = pytest.mark.gpu

MODES = ("fast", "exact")


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


@pytest.fixture(scope="module")
def bars(refcpu):
    """(8 KZ_ORACLE, 8 KX_ORACLE, 8 KN_ORACLE) and the oracle's maxima themselves."""
    ora = L.oracle_maxima()
    return tuple(BAR_FACTOR * v for v in ora), ora


@contextlib.contextmanager
def lrf_mode(mode):
    from se3icp import registration
    if mode == "exact":
        registration.set_lrf_exact(True)
    try:
        yield
    finally:
        registration.set_lrf_exact(False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", list(L.CASES))
def test_designed_cloud(se3icp_mod, bars, parity_record, kind, mode):
    (bz, bx, bn), ora = bars
    pts, idx = L.cloud(kind), L.knn_of(kind)
    got = {}
    with lrf_mode(mode):
        for k in L.CASES[kind]:
            got[k] = (se3icp_mod.knn_self(pts, k), se3icp_mod.toldi_frames(pts, k), se3icp_mod.estimate_normals(pts, k))
    top = {"kz": 0.0, "kx": 0.0, "kn": 0.0, "ydev": 0.0}
    fails = []
    for k, (knn, fr, nr) in got.items():
        parts, nref = L.case(kind, k)
        assert np.array_equal(knn, L.padded(idx, k)), (kind, mode, k, np.nonzero((knn != L.padded(idx, k)).any(1))[0][:8])
        assert np.isfinite(fr).all() and np.isfinite(nr).all(), (kind, mode, k)
        kz, kx, ydev, zsv = L.frame_measures(parts, fr)
        kn = L.normal_measure(nref, nr)
        print(f"[frames] {kind} {mode} k={k}: K_z {kz.max():.2f} (point {kz.argmax()})  K_x {kx.max():.2f} "
              f"({kx.argmax()})  K_n {kn.max():.2f} ({kn.argmax()})  |y - z x x| {ydev.max() / EPS:.2f} eps")
        for key, val, bar in (("kz", kz, bz), ("kx", kx, bx), ("kn", kn, bn), ("ydev", ydev, 4 * EPS)):
            top[key] = max(top[key], float(val.max()))
            if not val.max() <= bar:
                fails.append((k, key, float(val.max()), int(val.argmax()), bar))
        if not (zsv >= 0).all():
            fails.append((k, "z sign", np.nonzero(zsv < 0)[0][:8].tolist()))
        if not np.array_equal(fr[:, :3, 3].view(np.uint64), pts.view(np.uint64)):
            fails.append((k, "translation"))
        if not (np.array_equal(fr[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (len(pts), 4)))):
            fails.append((k, "last row"))
    parity_record(f"lrf frames: {kind} {mode}", points=len(pts), k_values=len(got), K_z=top["kz"], K_x=top["kx"],
                  K_n=top["kn"], y_dev_eps=top["ydev"] / EPS, K_z_oracle=ora[0], K_x_oracle=ora[1], K_n_oracle=ora[2])
    assert not fails, (kind, mode, fails)


# ------------------------------------------------------------------------------ exact cases
def _symmetric_set(h):
    """The 26 points {-h_a, 0, h_a}^3 without the origin: the sums of the coordinates and of the
    mixed products over the whole set are exactly zero, so the covariance is exactly diagonal."""
    g = np.array([[sx * h[0], sy * h[1], sz * h[2]] for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)
                  if (sx, sy, sz) != (0, 0, 0)], dtype=np.float64)
    return np.ascontiguousarray(g)


EXACT = {  # name: (cloud, k values, the normal of every point or None for "what the oracle returns")
    "extents 4 2 1": (_symmetric_set((4.0, 2.0, 1.0)), (26, 30), (0.0, 0.0, 1.0)),
    "extents 1 4 2": (_symmetric_set((1.0, 4.0, 2.0)), (26, 30), (1.0, 0.0, 0.0)),
    "extents 2 1 4": (_symmetric_set((2.0, 1.0, 4.0)), (26, 30), (0.0, 1.0, 0.0)),
    "extents 1 1 4": (_symmetric_set((1.0, 1.0, 4.0)), (26, 30), None),
    "extents 1 4 1": (_symmetric_set((1.0, 4.0, 1.0)), (26, 30), None),
    "32 copies": (np.ascontiguousarray(np.tile([[1.5, -2.25, 3.0625]], (32, 1))), (32, 40), (0.0, 0.0, 1.0)),
    "two points": (np.array([[0.5, 1.0, 1.5], [2.0, -1.0, 0.25]]), (2, 30), (0.0, 0.0, 1.0)),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_normals(se3icp_mod, refcpu, name, mode):
    """Every coordinate is a multiple of 2^-4 below 8.  With the whole cloud as the neighbourhood
    (k = n and k > n) the cumulants are exact; on the symmetric sets the off-diagonal
    covariances are exactly zero and FastEigen3x3 takes its diagonal branch:
    the normal is the axis of the smallest extent; with two equal smallest extents, what the
    oracle returns.  32 copies of one point give the zero covariance (mc == 0) and two points
    fewer than three neighbours: (0, 0, 1) both."""
    pts, ks, want = EXACT[name]
    assert (pts * 16 == np.round(pts * 16)).all() and np.abs(pts).max() < 8
    with lrf_mode(mode):
        got = {k: se3icp_mod.estimate_normals(pts, k) for k in ks}
    for k, g in got.items():
        ora = refcpu.estimate_normals(pts, k)
        print(f"[frames] exact {name} {mode} k={k}: {g[0]} (oracle {ora[0]})")
        if want is not None:
            assert np.array_equal(g, np.broadcast_to(np.array(want), g.shape)), (name, mode, k, g[:4])
        assert np.array_equal(g.view(np.uint64), ora.view(np.uint64)), (name, mode, k, g[:4], ora[:4])


@pytest.mark.parametrize("mode", MODES)
def test_exact_plane_normals(se3icp_mod, bars, parity_record, mode):
    """z = 0.25 exactly: the restatement's normal is e3 and the smallest eigenvalue 0; the
    normals are held to the K_n bar (which here bounds the tilt off e3)."""
    (_, _, bn), ora = bars
    pts = L.plane_cloud()
    idx = L.knn_ld(pts, L.K_MAX)
    with lrf_mode(mode):
        got = {k: se3icp_mod.estimate_normals(pts, k) for k in L.K_512}
    top = 0.0
    for k, nr in got.items():
        nref = L.normals_ld(pts, idx, k)
        assert np.array_equal(np.abs(nref[0].astype(np.float64)), np.broadcast_to([0.0, 0.0, 1.0], nr.shape)), k
        assert np.isfinite(nr).all(), k
        kn = L.normal_measure(nref, nr)
        print(f"[frames] plane {mode} k={k}: K_n {kn.max():.2f} (point {kn.argmax()}), "
              f"largest tilt {np.abs(nr[:, :2]).max():.2e}")
        top = max(top, float(kn.max()))
        assert kn.max() <= bn, (mode, k, float(kn.max()), int(kn.argmax()), bn)
    parity_record(f"lrf frames: plane {mode}", points=len(pts), k_values=len(got), K_n=top, K_n_oracle=ora[2])
