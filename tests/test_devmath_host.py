"""CPU tests of gicp_cov_from_normal (se3-icp_amd/csrc/devmath.hpp), the covariance k_reduce
rebuilds from the stored normal of every GICP correspondence.  The function is
__host__ __device__ plain arithmetic, so the same source is built here for the host
(tests/devmath_host.cpp) and checked against the oracle's GetRotationFromE1ToX /
R diag(eps, 1, 1) R^T (refcpu.gicp_covariances) and the long-double restatement cov_ld.

The function has one discontinuous branch: R = I when n.x < -0.99 (ISR.cpp:4-14).  No normal
of the suite's clouds takes it (Open3D's FastEigen3x3 returns the eigenvector of a planar
neighbourhood as a cross product of two rows of A - lambda I whose dominant component is a
principal 2 x 2 minor of a positive semi-definite matrix, hence positive: a normal within 8
degrees of the x axis always points along +x), so it is reached here,
with normals given directly on both sides of the threshold.

Both sides compile the same operations in the same order without FMA contraction (the
function under `#pragma clang fp contract(off)`, the oracle with -ffp-contract=off), so the
comparison with the oracle is bitwise.

The two eigen-solvers of the setup kernels (jacobi_smallest_evec: the TOLDI z axis;
fast_eigen3x3: the normals) are __host__ __device__ too, and the same program's `eig` mode runs
them on matrices Q diag(lambda) Q^T of prescribed spectra (SPECTRA): both signs of
FastEigen3x3's half_det, gaps down to 1e-12, a zero smallest eigenvalue, three scales, diagonal
input in every order (the nrm == 0 branch) and the zero matrix (mc == 0).  The measure is the
angle to the long-double eigenvector of the f64 matrix in units of eps |A|_F / gap, the
first-order bound of an eigenvector's movement under a rounding of the matrix; each solver is
held to 8 x what the oracle's solver (refcpu.sym_eig3_smallest / refcpu.fast_eigen3x3: the
same algorithms without FMA contraction) reaches on the same matrices."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_steps import LD, cov_ld, unit_normals

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UPPER = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])  # xx xy xz yy yz zz


@pytest.fixture(scope="module")
def refcpu():
    from oracle import refcpu as r
    r.lib()
    return r


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("dm") / "devmath_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "se3-icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "devmath_host.cpp"), "-o", exe])

    def run(rows, *args):
        text = "".join(" ".join(float(v).hex() for v in r) + "\n" for r in rows)
        out = subprocess.run([exe, *args], input=text, capture_output=True, text=True, check=True)
        got = [[float.fromhex(t) for t in ln.split()] for ln in out.stdout.strip().splitlines()]
        assert len(got) == len(rows)
        return np.array(got)
    return run


@pytest.fixture(scope="module")
def host_cov(host_exe):
    return host_exe


@pytest.fixture(scope="module")
def host_eig(host_exe):
    """(jacobi_smallest_evec, fast_eigen3x3) of rows a00 a01 a02 a11 a12 a22: two (n, 3) arrays."""
    def run(a6):
        out = host_exe(a6, "eig")
        return out[:, :3], out[:, 3:]
    return run


def _with_nx(c):
    """The unit normal (c, s cos 1, s sin 1), s = sqrt(1 - c^2), with n.x exactly c."""
    s = np.sqrt(1.0 - c * c)
    return [c, s * np.cos(1.0), s * np.sin(1.0)]


THRESHOLD = -0.99
BELOW, ABOVE = np.nextafter(THRESHOLD, -1.0), np.nextafter(THRESHOLD, 0.0)


def special_normals():
    axes = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    return np.array(axes + [_with_nx(BELOW), _with_nx(THRESHOLD), _with_nx(ABOVE), _with_nx(-1.0 + 2.0 ** -52)], dtype=np.float64)


def test_host_covariances_equal_the_oracle_bitwise(host_cov, refcpu):
    nrm = np.concatenate([special_normals(), unit_normals(1000, 9)])
    taken = nrm[:, 0] < THRESHOLD
    assert taken.tolist()[:10] == [False, True, False, False, False, False, True, False, False, True]
    assert 1 <= int(taken[10:].sum()) <= 20  # (the cap within 8.1 degrees of -e1: 0.5 % of the sphere)
    got = host_cov(nrm)
    want = refcpu.gicp_covariances(nrm)[:, UPPER[0], UPPER[1]]
    assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), \
        np.nonzero((got != want).any(1))[0][:8]
    dev = float(np.abs(got.astype(LD) - cov_ld(nrm)[:, UPPER[0], UPPER[1]]).max())
    print(f"[devmath] host gicp_cov_from_normal against long double: {dev:.2e} over {len(nrm)} normals, "
          f"{int(taken.sum())} on the R = I branch")
    assert dev <= 1e-15


def test_the_branch_and_its_jump(host_cov):
    """n.x < -0.99 gives diag(eps, 1, 1) exactly; -0.99 itself and everything above take the
    formula, which for a unit normal gives I - (1 - eps) n n^T.  Across the threshold the
    covariance therefore jumps by that difference: (1 - eps) (1 - 0.99^2) = 0.0199 in xx."""
    eps = 1e-3
    sp = special_normals()
    got = host_cov(sp)
    flat = np.array([eps, 0.0, 0.0, 1.0, 0.0, 1.0])
    for i in (1, 6, 9):  # -e1, one step below -0.99, -1 + 2^-52
        assert np.array_equal(got[i], flat), (i, got[i])
    for i in (0, 2, 3, 4, 5, 7, 8):  # the formula: a rotation taking e1 to n
        n = sp[i].astype(LD)
        want = (np.eye(3, dtype=LD) - (1 - LD(eps)) * np.outer(n, n))[UPPER]
        assert float(np.abs(got[i] - want).max()) <= 1e-13, (i, got[i], want)  # (1 / (1 + n.x) = 100 at the threshold)
    assert np.array_equal(got[0], flat)  # +e1: R = I by the formula
    jump = got[7] - got[6]  # exactly -0.99 (formula) against one step below (R = I)
    n = sp[7].astype(LD)
    want = (-(1 - LD(eps)) * np.outer(n, n))[UPPER] + np.array([1 - LD(eps), 0, 0, 0, 0, 0], LD)
    assert float(np.abs(jump - want).max()) <= 1e-13
    assert abs(jump[0] - (1 - eps) * (1 - 0.99 ** 2)) <= 1e-13 and abs(jump[0]) > 0.019
    # one step above the threshold is the formula's neighbour: continuous there
    assert float(np.abs(got[8] - got[7]).max()) <= 1e-13


# =========================================================================== the eigen-solvers
EPS = 2.0 ** -52
N_Q = 200


def _spectra():
    base = [("1 2 3", (1.0, 2.0, 3.0))]
    for j in range(2, 13):
        base.append((f"1 1+1e-{j} 3", (1.0, 1.0 + 10.0 ** -j, 3.0)))   # half_det > 0: the top one apart
        base.append((f"1 3-1e-{j} 3", (1.0, 3.0 - 10.0 ** -j, 3.0)))   # half_det < 0: the smallest apart
    base += [("0 1 1", (0.0, 1.0, 1.0)), ("1e-6 1 1", (1e-6, 1.0, 1.0))]
    return [(f"{name} x {sc:g}", tuple(sc * v for v in lam)) for sc in (1.0, 1e-12, 1e12) for name, lam in base]


SPECTRA = _spectra()
REPEATED = [(f"1 1 3 x {sc:g}", (sc, sc, 3 * sc)) for sc in (1.0, 1e-12, 1e12)]  # the smallest one repeated


def _rotations_ld(n, seed):
    """n rotation matrices from unit quaternions normalised in long double."""
    q = np.random.default_rng(seed).standard_normal((n, 4)).astype(LD)
    q /= np.sqrt((q * q).sum(1))[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def _sym6(A):
    return np.ascontiguousarray(np.asarray(A)[:, UPPER[0], UPPER[1]], dtype=np.float64)


def _full(a6):
    A = np.zeros((len(a6), 3, 3))
    A[:, UPPER[0], UPPER[1]] = a6
    A[:, UPPER[1], UPPER[0]] = a6
    return A


@pytest.fixture(scope="module")
def spectra_matrices():
    """{name: a6 (N_Q, 6) f64}: Q diag(lambda) Q^T in long double, rounded to f64; one set of
    rotations per spectrum."""
    out = {}
    for i, (name, lam) in enumerate(SPECTRA + REPEATED):
        Q = _rotations_ld(N_Q, 100 + i)
        out[name] = _sym6(np.einsum("nab,b,ncb->nac", Q, np.array(lam, LD), Q))
    return out


def _angle_measure(a6, vec):
    """angle(vec, long-double eigenvector of the f64 matrix) gap / (eps |A|_F) per matrix."""
    from lrf_reference import jacobi_eigh_ld
    A = _full(a6).astype(LD)
    lam, V = jacobi_eigh_ld(A)
    v0 = V[:, :, 0]
    g = np.asarray(vec, dtype=np.float64).astype(LD)
    sin = np.sqrt((np.cross(g, v0) ** 2).sum(1)) / np.sqrt((g * g).sum(1))
    cos = np.abs((g * v0).sum(1)) / np.sqrt((g * g).sum(1))
    ang = np.arctan2(sin, cos)
    nrm = np.sqrt((A * A).sum((1, 2)))
    return (ang * (lam[:, 1] - lam[:, 0]) / (EPS * nrm)).astype(np.float64)


def test_eigen_solvers_on_prescribed_spectra(host_eig, refcpu, spectra_matrices):
    fails = []
    top = {"jacobi": (0.0, 0.0, ""), "fast": (0.0, 0.0, "")}
    for name, _ in SPECTRA:
        a6 = spectra_matrices[name]
        hj, hf = host_eig(a6)
        oj, of = refcpu.sym_eig3_smallest(a6), refcpu.fast_eigen3x3(a6)
        assert np.isfinite(hj).all() and np.isfinite(hf).all(), name
        for solver, h, o in (("jacobi", hj, oj), ("fast", hf, of)):
            mh, mo = float(_angle_measure(a6, h).max()), float(_angle_measure(a6, o).max())
            if mh > top[solver][0]:
                top[solver] = (mh, mo, name)
            if not mh <= 8 * mo:
                fails.append((solver, name, mh, mo))
    for solver, (mh, mo, name) in top.items():
        print(f"[devmath] {solver}: largest angle gap / (eps |A|) {mh:.2f} (oracle {mo:.2f}) on '{name}', "
              f"{len(SPECTRA)} spectra x {N_Q} rotations")
    assert not fails, fails


def test_eigen_solvers_where_the_smallest_eigenvalue_repeats(host_eig, spectra_matrices):
    """The vector is undefined within the eigenplane: it must be finite, of unit length, and
    have the smallest eigenvalue as its Rayleigh quotient."""
    from lrf_reference import jacobi_eigh_ld
    for name, _ in REPEATED:
        a6 = spectra_matrices[name]
        A = _full(a6).astype(LD)
        lam0 = jacobi_eigh_ld(A)[0][:, 0]
        nrm = np.sqrt((A * A).sum((1, 2)))
        for solver, h in zip(("jacobi", "fast"), host_eig(a6)):
            assert np.isfinite(h).all(), (name, solver)
            g = h.astype(LD)
            unit = np.abs(np.sqrt((g * g).sum(1)) - 1)
            ray = np.abs(np.einsum("na,nab,nb->n", g, A, g) - lam0) / nrm
            print(f"[devmath] {solver} on '{name}': | |v| - 1 | {float(unit.max()) / EPS:.2f} eps, "
                  f"|v.Av - lambda_0| {float(ray.max()) / EPS:.2f} eps |A|")
            assert unit.max() <= 4 * EPS, (name, solver, float(unit.max()))
            assert ray.max() <= 64 * EPS, (name, solver, float(ray.max()))


def test_eigen_solvers_on_diagonal_and_zero_input(host_eig, refcpu):
    """Diagonal input in every order and at every scale (FastEigen3x3's nrm == 0 branch, Jacobi
    without a rotation) and the zero matrix (mc == 0: FastEigen3x3 returns the zero vector, which
    its callers replace by e3): the host vectors are the oracle's, bit for bit, and the axis of
    the smallest entry where there is one."""
    import itertools
    rows, want = [], []
    for _, lam in SPECTRA + REPEATED:
        for perm in itertools.permutations(range(3)):
            d = [lam[p] for p in perm]
            rows.append([d[0], 0.0, 0.0, d[1], 0.0, d[2]])
            lo = [i for i in range(3) if d[i] == min(d)]
            want.append(lo[0] if len(lo) == 1 else -1)
    rows.append([0.0] * 6)
    want.append(-1)
    a6 = np.array(rows)
    hj, hf = host_eig(a6)
    oj, of = refcpu.sym_eig3_smallest(a6), refcpu.fast_eigen3x3(a6)
    assert np.array_equal(hj.view(np.uint64), oj.view(np.uint64)), np.nonzero((hj != oj).any(1))[0][:8]
    assert np.array_equal(hf.view(np.uint64), of.view(np.uint64)), np.nonzero((hf != of).any(1))[0][:8]
    for i, ax in enumerate(want):
        if ax >= 0:
            assert np.array_equal(np.abs(hj[i]), np.eye(3)[ax]) and np.array_equal(hf[i], np.eye(3)[ax]), (i, rows[i])
    assert np.array_equal(hf[-1], np.zeros(3)) and np.array_equal(hj[-1], [1.0, 0.0, 0.0])
