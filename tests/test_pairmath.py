"""CPU tests of se3-icp_amd/csrc/pairmath.hpp, the per-pair f64 solve and loop state
machine that k_reduce_final runs on the GPU (ISR.cpp:684-732).  The header is
__host__ __device__, so the same source is built here for the host (tests/pairmath_host.cpp)
and checked against numpy restatements of the reference's estimator semantics:
Eigen::umeyama without scaling (ISR.cpp:692), Open3D's LDLT solve of JTJ x = -JTr with
TransformVector6dToMatrix4d (ISR.cpp:695-698, 101-107), and the switch / convergence tests
(ISR.cpp:547-550, 718-729, 1118-1119)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def pairmath(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("pm") / "pairmath_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "se3-icp_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pairmath_host.cpp"),
                           "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
        return [np.array([float(x) for x in ln.split()]) for ln in out.stdout.strip().splitlines()]
    return run


def _fmt(vals):
    return " ".join(repr(float(v)) for v in vals)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _moments(src, dst):
    return np.concatenate([src.sum(0), dst.sum(0), (dst.T @ src).reshape(-1)]), float(src.shape[0])


def _umeyama(src, dst):
    ms, md = src.mean(0), dst.mean(0)
    sigma = (dst - md).T @ (src - ms) / src.shape[0]
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = md - R @ ms
    return T


def test_umeyama_matches_numpy_and_recovers_exact_motion(pairmath):
    rng = np.random.default_rng(5)
    cases, want = [], []
    for i in range(20):
        src = rng.normal(size=(200, 3)) * rng.uniform(0.5, 3.0)
        R = _rot(*rng.uniform(-np.pi, np.pi, 3))
        t = rng.uniform(-5, 5, 3)
        dst = src @ R.T + t + (rng.normal(scale=0.05, size=src.shape) if i % 2 else 0.0)
        s, n = _moments(src, dst)
        cases.append("U " + _fmt(s) + " " + _fmt([n]))
        want.append(_umeyama(src, dst))
        if i % 2 == 0:  # noise-free: the motion itself
            assert np.allclose(want[-1][:3, :3], R, atol=1e-9) and np.allclose(want[-1][:3, 3], t, atol=1e-9)
    for got, T in zip(pairmath(cases), want):
        assert np.abs(got.reshape(4, 4) - T).max() < 1e-9
    # reflection case (det(U) det(V) < 0 is corrected to a rotation) and n = 0 (identity)
    src = rng.normal(size=(50, 3))
    dst = src * np.array([1.0, 1.0, -1.0])
    s, n = _moments(src, dst)
    got = pairmath(["U " + _fmt(s) + " " + _fmt([n]), "U " + _fmt(np.zeros(15)) + " 0"])
    assert np.isclose(np.linalg.det(got[0].reshape(4, 4)[:3, :3]), 1.0)
    assert np.abs(got[0].reshape(4, 4) - _umeyama(src, dst)).max() < 1e-9
    assert np.array_equal(got[1].reshape(4, 4), np.eye(4))


def test_umeyama_rotation_extremes(pairmath):
    """The Jacobi rotations of the 3x3 SVD come from half-angle formulas, not trigonometric
    calls: half turns (cos 2t = -1 blocks), quarter turns, near-identity motions and a planar
    source (rank-2 cross-covariance) must still give numpy's umeyama."""
    rng = np.random.default_rng(11)
    cases, want = [], []
    rots = [np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0]), np.diag([-1.0, 1.0, -1.0]),
            _rot(0, 0, np.pi / 2), _rot(np.pi / 2, 0, 0), _rot(0, np.pi - 1e-9, 0), _rot(1e-9, -2e-9, 3e-9),
            _rot(np.pi, np.pi / 2, -np.pi / 3)]
    for i, R in enumerate(rots):
        src = rng.normal(size=(100, 3)) * np.array([2.0, 1.0, 0.5])
        if i == len(rots) - 1:
            src[:, 2] = 0.0  # planar source
        t = rng.uniform(-1, 1, 3)
        dst = src @ R.T + t
        s, n = _moments(src, dst)
        cases.append("U " + _fmt(s) + " " + _fmt([n]))
        want.append(_umeyama(src, dst))
        assert np.allclose(want[-1][:3, :3], R, atol=1e-7)
    for got, T in zip(pairmath(cases), want):
        G = got.reshape(4, 4)
        assert np.abs(G - T).max() < 1e-9, (G, T)
        assert np.isclose(np.linalg.det(G[:3, :3]), 1.0)


@pytest.mark.parametrize("scale", [1e-85, 1e85])
def test_umeyama_tiny_and_huge_cross_covariance(pairmath, scale):
    """Cross-covariance entries around 1e-170 and 1e170: the Jacobi
    hypotenuses must neither underflow to a 0/0 rotation nor overflow to a zeroed block."""
    rng = np.random.default_rng(13)
    cases, want, rots = [], [], []
    for _ in range(6):
        R = _rot(*rng.uniform(-np.pi, np.pi, 3))
        src = rng.normal(size=(100, 3)) * np.array([2.0, 1.0, 0.5]) * scale
        dst = src @ R.T + rng.uniform(-1, 1, 3) * scale
        s, n = _moments(src, dst)
        cases.append("U " + _fmt(s) + " " + _fmt([n]))
        want.append(_umeyama(src, dst))
        rots.append(R)
    for got, T, R in zip(pairmath(cases), want, rots):
        G = got.reshape(4, 4)
        assert np.all(np.isfinite(G)), G
        assert np.abs(G[:3, :3] - R).max() < 1e-9, (G, R)
        assert np.abs(G[:3, 3] - T[:3, 3]).max() < 1e-9 * scale, (G, T)


def _pack(A, b):
    return np.concatenate([A[np.triu_indices(6)], b])


def _vec6(x):
    T = np.eye(4)
    T[:3, :3] = _rot(x[0], x[1], x[2])  # Rz(x2) Ry(x1) Rx(x0)
    T[:3, 3] = x[3:]
    return T


def test_normal_equations_match_numpy_ldlt_semantics(pairmath):
    rng = np.random.default_rng(7)
    cases, want = [], []
    for _ in range(20):
        J = rng.normal(size=(40, 6))
        A = J.T @ J
        b = rng.normal(size=6)
        cases.append("N " + _fmt(_pack(A, b)))
        want.append(_vec6(np.linalg.solve(A, -b)))
    # rank-deficient (a zero pivot is skipped: that component of x is 0, Eigen LDLT)
    A = np.diag([2.0, 3.0, 4.0, 5.0, 6.0, 0.0])
    b = np.array([1.0, -1.0, 2.0, 0.5, -0.5, 0.0])
    cases.append("N " + _fmt(_pack(A, b)))
    x = np.zeros(6)
    x[:5] = -b[:5] / np.diag(A)[:5]
    want.append(_vec6(x))
    # all-zero system (no correspondences kept): identity
    cases.append("N " + _fmt(np.zeros(27)))
    want.append(np.eye(4))
    for got, T in zip(pairmath(cases), want):
        assert np.abs(got.reshape(4, 4) - T).max() < 1e-9
    # a non-finite solution returns the identity (ISR.cpp:101-107, Open3D's failure path)
    nan_case = _pack(np.eye(6), np.full(6, np.nan))
    assert np.array_equal(pairmath(["N " + _fmt(nan_case)])[0].reshape(4, 4), np.eye(4))


def _state_case(T, kind, est, sw, it, max_iter, max_se3, mse, mse_switch, sf, K, mse_cur, acc):
    return "S " + _fmt(np.asarray(T).reshape(-1)) + f" {kind} {est} {sw} {it} {max_iter} {max_se3} " + \
        _fmt([mse, mse_switch, sf, K, mse_cur]) + " " + _fmt(acc)


def test_switch_and_convergence_state_machine(pairmath):
    I = np.eye(4)
    zero = np.zeros(28)
    move = np.zeros(28)  # pt2pl system whose solution moves the pose by 0.1 along x
    move[0:21] = np.eye(6)[np.triu_indices(6)]
    move[21 + 3] = -0.1

    def acc_with(base, mse_sum):
        a = base.copy()
        a[27] = mse_sum
        return a
    KIND_ICP, KIND_SE3, KIND_PURE = 0, 1, 3
    PT2PL = 1
    out = pairmath([
        # SE(3) phase, no pose change -> switch (change < mse_switch, ISR.cpp:718-723)
        _state_case(I, KIND_SE3, PT2PL, 0, 3, 150, 10, 1e-5, 5e-5, 0.5, 100, 2.0, acc_with(zero, 150.0)),
        # SE(3) phase, moving, at max_num_se3_iterations -> switch
        _state_case(I, KIND_SE3, PT2PL, 0, 10, 150, 10, 1e-5, 5e-5, 0.5, 100, 2.0, acc_with(move, 150.0)),
        # SE(3) phase, moving, below the cap -> stays in the SE(3) phase
        _state_case(I, KIND_SE3, PT2PL, 0, 4, 150, 10, 1e-5, 5e-5, 0.5, 100, 2.0, acc_with(move, 150.0)),
        # R3 phase, mse unchanged -> done (rel < sf * mse, ISR.cpp:724-729)
        _state_case(I, KIND_SE3, PT2PL, 1, 20, 150, 10, 1e-5, 5e-5, 0.5, 100, 1.5, acc_with(move, 150.0)),
        # R3 phase, mse still moving -> continues
        _state_case(I, KIND_SE3, PT2PL, 1, 20, 150, 10, 1e-5, 5e-5, 0.5, 100, 2.0, acc_with(move, 150.0)),
        # run_icp: iter == max_num_iterations -> done (ISR.cpp:547-550, `==`)
        _state_case(I, KIND_ICP, PT2PL, 0, 7, 7, 10, 1e-5, 5e-5, 1.0, 100, 2.0, acc_with(move, 150.0)),
        # run_se3_pure: iter == max_num_se3_iterations -> done (ISR.cpp:1118-1119)
        _state_case(I, KIND_PURE, PT2PL, 0, 10, 150, 10, 1e-5, 5e-5, 0.5, 100, 2.0, acc_with(move, 150.0)),
    ])
    iter_, pure, sw, done, phase, pstart, mse_cur, rel = [np.array([o[i] for o in out]) for i in range(8)]
    T = [o[8:].reshape(4, 4) for o in out]
    assert list(sw) == [1, 1, 0, 1, 1, 0, 0]
    assert list(done) == [0, 0, 0, 1, 0, 1, 1]
    # the next iteration is opened for the live pairs: R3 after a switch, SE(3) otherwise
    assert list(phase) == [2, 2, 1, 0, 2, 0, 0]
    assert list(iter_) == [4, 11, 5, 20, 21, 7, 10]
    assert pstart[0] == 4 and pstart[1] == 11 and pstart[2] == 1
    assert np.allclose(mse_cur, 1.5) and np.allclose(rel[0], 0.5)
    assert np.allclose(T[1][:3, 3], [0.1, 0, 0]) and np.allclose(T[0], I)


def _umeyama_ld(src, dst):
    """Two-pass centred umeyama in long double (the SVD in f64 of the long-double sigma,
    polished by one long-double orthogonalisation step; translation in long double)."""
    ld = np.longdouble
    s, d = src.astype(ld), dst.astype(ld)
    ms, md = s.sum(0) / ld(len(s)), d.sum(0) / ld(len(d))
    sigma = (d - md).T @ (s - ms) / ld(len(s))
    U, _, Vt = np.linalg.svd(sigma.astype(np.float64))
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = (U @ S @ Vt).astype(ld)
    # the polar factor of sigma is the fixed point of R <- R (3 I - R^T R) / 2 restricted to
    # the f64 SVD's rounding: one step takes the f64 result's 1e-16 departure from orthogonality to 1e-32
    R = R @ (ld(3) * np.eye(3, dtype=ld) - R.T @ R) / ld(2)
    return R, md - R @ ms


PIVOT_OFFSETS = [0.0, 1e3, 1e5, 1e6, 1e7]


@pytest.mark.parametrize("offset", PIVOT_OFFSETS)
def test_umeyama_moments_about_a_pivot_off_origin(pairmath, offset):
    """4000 points of spread 30 at `offset` from the origin, exact (long-double, rounded once)
    moments.  Raw moments (the U case: what k_reduce summed before the pivot) lose
    eps (offset / spread)^2 against the long-double centred umeyama; measured with this input:

      offset   rotation error   max point displacement
      0        4e-16            5e-14
      1e3      2e-14            3e-12
      1e5      5e-10            8e-8
      1e6      3e-8             4e-6
      1e7      4e-6             5e-4

    (a less favourable draw loses a hundred times more: 2e-8 and 3e-6 at 1e5.)  Moments about
    the target centroid, un-shifted by pair_close_iteration (the P case), must stay at the
    offset-0 level: rotation within 1e-14 (sigma's entries carry a few eps relative error at
    any offset, and the cloud is well conditioned), and every point within
    1e-13 * spread + 16 eps * offset of the reference's image (the second term is the f64
    representation of a translation of size ~2 * offset and the three rounded products of
    R c; the displacement is evaluated in long double).  Measured: rotation 2e-16 .. 6e-16,
    displacement 7e-14 / 1e-13 / 1e-11 / 8e-11 / 4e-10."""
    ld = np.longdouble
    rng = np.random.default_rng(41)
    n, spread = 4000, 30.0
    base = rng.normal(size=(n, 3)) * spread
    R0 = _rot(0.3, -0.2, 0.4)
    c = offset * np.array([0.6, -0.7, 0.4]) / np.linalg.norm([0.6, -0.7, 0.4])
    src = base + c
    dst = base @ R0.T + rng.normal(scale=0.05, size=base.shape) + np.array([1.0, -2.0, 0.5]) + c
    Rr, tr = _umeyama_ld(src, dst)
    piv = dst.mean(0)

    def moments(p):
        s, d = src.astype(ld) - p.astype(ld), dst.astype(ld) - p.astype(ld)
        return np.concatenate([s.sum(0), d.sum(0), (d.T @ s).reshape(-1)]).astype(np.float64)
    raw, piv_out = pairmath(["U " + _fmt(moments(np.zeros(3))) + f" {n}",
                             "P " + _fmt(piv) + " " + _fmt(moments(piv)) + f" {n}"])

    def defect(T):
        T = T.reshape(4, 4).astype(ld)
        disp = src.astype(ld) @ (T[:3, :3] - Rr).T + (T[:3, 3] - tr)
        return float(np.abs(T[:3, :3] - Rr).max()), float(np.sqrt((disp ** 2).sum(1)).max())
    (r_raw, d_raw), (r_piv, d_piv) = defect(raw), defect(piv_out)
    print(f"[pivot] offset {offset:g}: raw moments rotation {r_raw:.1e} displacement {d_raw:.1e}; "
          f"about the pivot rotation {r_piv:.1e} displacement {d_piv:.1e}")
    eps = 2.0 ** -52
    assert r_piv <= 1e-14, (offset, r_piv)
    assert d_piv <= 1e-13 * spread + 16 * eps * offset, (offset, d_piv)
    if offset == 0.0:  # a zero pivot is skipped: the closing step is umeyama_from_moments' result itself
        zero = pairmath(["P 0 0 0 " + _fmt(moments(np.zeros(3))) + f" {n}"])[0]
        assert np.array_equal(zero, raw)
