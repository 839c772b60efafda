"""CPU tests of the long-double restatement of the setup stage (lrf_reference.py) and of what
the GPU tests of test_gpu_frames.py are made of:

  * the restatement's Jacobi against mpmath at 40 digits, on matrices of the designed clouds,
    the smallest eigen-gaps included;
  * the oracle (oracle/refcpu.cpp, f64, sequential sums) against the restatement on every
    (kind, k): its largest K_z, K_x, K_n are what the engine's bars are multiples of;
  * the design conditions: on these clouds no point is ill-conditioned, so no point is left
    out of any comparison;
  * the power of the measures: each planted defect of the restatement (a wrong rank range,
    divisor, radius, weight, or the self point left out) puts the oracle more than three
    orders above the engine's bar.
"""
import mpmath
import numpy as np
import pytest

import lrf_reference as L
from lrf_reference import BAR_FACTOR, EPS, LD


@pytest.fixture(scope="module")
def refcpu():
    from oracle import refcpu as r
    r.lib()
    return r


@pytest.fixture(scope="module")
def measures(refcpu):
    return L.oracle_measures()


def _mp(x):
    """A long double as an exact mpf (its 64-bit mantissa as two f64 parts)."""
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - LD(hi)))


def _design_matrices():
    """About 50 symmetric matrices of the designed clouds: the TOLDI covariances with the
    smallest relative gaps of all cases, and a spread of TOLDI and normal covariances."""
    rows = []
    for kind, ks in L.CASES.items():
        for k in ks:
            parts, _ = L.case(kind, k)
            rel = parts["gap"] / parts["lam"][:, 2]
            for i in np.argsort(rel)[:2]:
                rows.append((float(rel[i]), parts["C"][i]))
    rows.sort(key=lambda r: r[0])
    mats = [c for _, c in rows[:30]] + [c for _, c in rows[30::8]][:10]
    pts = L.cloud("offset")
    P = pts.astype(LD)
    nb = P[L.knn_of("offset")[::47, :30]]
    d = nb - nb.mean(1)[:, None, :]
    mats += list(np.einsum("nki,nkj->nij", d, d) / LD(30))
    return np.array(mats, dtype=LD)


def test_long_double_jacobi_matches_mpmath():
    mats = _design_matrices()
    assert 45 <= len(mats) <= 60
    lam, V = L.jacobi_eigh_ld(mats)
    worst_vec = worst_val = 0.0
    smallest_rel_gap = np.inf
    with mpmath.workdps(40):
        for A, w, v in zip(mats, lam, V):
            E, Q = mpmath.eigsy(mpmath.matrix([[_mp(A[i, j]) for j in range(3)] for i in range(3)]))
            order = sorted(range(3), key=lambda i: E[i])
            e = [E[i] for i in order]
            q0 = [Q[r, order[0]] for r in range(3)]
            norm = mpmath.sqrt(sum(_mp(x) ** 2 for x in A.ravel()))
            gap = e[1] - e[0]
            smallest_rel_gap = min(smallest_rel_gap, float(gap / e[2]))
            sign = 1 if sum(q0[r] * _mp(v[r, 0]) for r in range(3)) >= 0 else -1
            dv = mpmath.sqrt(sum((sign * q0[r] - _mp(v[r, 0])) ** 2 for r in range(3)))
            dw = max(abs(e[c] - _mp(w[c])) for c in range(3))
            tol = 64 * mpmath.mpf(2) ** -63 * norm
            worst_vec = max(worst_vec, float(dv * gap / tol))
            worst_val = max(worst_val, float(dw / tol))
            assert dv <= tol / gap, (float(dv), float(tol / gap))
            assert dw <= tol, (float(dw), float(tol))
    print(f"[lrf] long-double Jacobi against mpmath on {len(mats)} matrices (smallest relative gap "
          f"{smallest_rel_gap:.1e}): vector {worst_vec:.3f}, values {worst_val:.3f} of the allowed 64 x 2^-63 |C| / gap")
    assert smallest_rel_gap < 1e-7  # the hard ones are in


def test_brute_force_lists_equal_the_oracle(refcpu):
    for kind in L.CASES:
        idx = L.knn_of(kind)
        ri, rd = refcpu.knn_self(L.cloud(kind), idx.shape[1])
        assert np.array_equal(idx, ri), kind
        assert (idx[:, 0] == np.arange(len(idx))).all(), kind
        assert (np.diff(rd, axis=1) > 0).all(), kind  # no ties: the lists are unique


def test_design_conditions(measures):
    """Asserted on the restatement and the oracle alone, every point of every case."""
    worst = {"gap": np.inf, "ngap": np.inf, "x": np.inf, "sign": np.inf}
    for (kind, k), m in measures.items():
        parts, nref = L.case(kind, k)
        rel = parts["gap"] / parts["lam"][:, 2]
        nrel = nref[1] / nref[3][:, 2]
        _, xr, sw = L.toldi_x(parts, parts["z"])
        margin = np.abs((parts["z"] * parts["sv"]).sum(1)) / (EPS * parts["sabs_v"])
        assert rel.min() > 1e-10, (kind, k, float(rel.min()))
        assert nrel.min() > 1e-10, (kind, k, float(nrel.min()))
        assert (xr / sw).min() > 1e-4, (kind, k, float((xr / sw).min()))
        assert margin.min() > 1e6, (kind, k, float(margin.min()))
        for key, val in (("gap", rel), ("ngap", nrel), ("x", xr / sw), ("sign", margin)):
            worst[key] = min(worst[key], float(val.min()))
    print(f"[lrf] smallest relative gap {worst['gap']:.1e} (frames) {worst['ngap']:.1e} (normals), "
          f"x-axis ratio {worst['x']:.1e}, z-sign margin {worst['sign']:.1e} eps")


def test_oracle_against_restatement(measures):
    """The oracle rounds like f64: a sequential sum of m products is within m eps of the sum of
    their magnitudes, and the eigenvector and the x axis inherit that through gap and |x_raw|, so
    every measure is below the number of neighbours summed plus a few units for forming the
    terms and the solver.  Its axes are a frame, and its translation is the point."""
    for (kind, k), m in measures.items():
        pts = L.cloud(kind)
        kk = min(k, len(pts))
        for key in ("kz", "kx", "kn"):
            assert np.isfinite(m[key]).all(), (kind, k, key)
            assert m[key].max() <= kk + 16, (kind, k, key, float(m[key].max()))
        assert m["ydev"].max() <= 4 * EPS, (kind, k)
        assert (m["zsv"] >= 0).all(), (kind, k)
        assert np.array_equal(m["frames"][:, :3, 3], pts), (kind, k)
    kz, kx, kn = L.oracle_maxima()
    print(f"[lrf] oracle maxima over {len(measures)} (kind, k): K_z {kz:.2f}  K_x {kx:.2f}  K_n {kn:.2f}")
    for kind in L.CASES:
        print(f"[lrf]   {kind}: " + "  ".join(f"{v:.2f}" for v in L.oracle_maxima(kind)))
    # the engine's bars are 8 x these, so they must not drift up unseen: rounding errors of m <= 150
    # terms add in quadrature (sqrt(150) = 12.2), times the two or three roundings that form a term
    assert max(kz, kx, kn) <= 32


AFFECTED = {"cov_ranks": "kz", "centroid_div": "kz", "radius_rank": "kx", "weight_unsq": "kx", "no_self": "kn"}


@pytest.mark.parametrize("defect", L.DEFECTS)
@pytest.mark.parametrize("k", [30, 25])
def test_planted_defects_are_three_orders_over_the_bar(measures, defect, k):
    pts, idx = L.cloud("surface"), L.knn_of("surface")
    m = measures[("surface", k)]
    key = AFFECTED[defect]
    if key == "kn":
        got = L.normal_measure(L.normals_ld(pts, idx, k, (defect,)), m["normals"])
    else:
        kz, kx, _, _ = L.frame_measures(L.toldi_z(pts, idx, k, (defect,)), m["frames"])
        got = kz if key == "kz" else kx
    bar = BAR_FACTOR * dict(zip(("kz", "kx", "kn"), L.oracle_maxima()))[key]
    med = float(np.median(got))
    print(f"[lrf] defect {defect} at k={k}: median {key} {med:.2e}, bar {bar:.1f}")
    assert med > 1e3 * bar, (defect, k, med, bar)
