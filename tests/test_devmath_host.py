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
comparison with the oracle is bitwise."""
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
def host_cov(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("dm") / "devmath_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", os.path.join(ROOT, "se3-icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "devmath_host.cpp"), "-o", exe])

    def run(normals):
        text = "".join(" ".join(float(v).hex() for v in n) + "\n" for n in normals)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        rows = [[float.fromhex(t) for t in ln.split()] for ln in out.stdout.strip().splitlines()]
        assert len(rows) == len(normals)
        return np.array(rows)
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
