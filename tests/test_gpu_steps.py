"""The Jacobian estimators of k_loop.hip (corr_terms' pt2pl, GICP and confidence-weighted GICP
branches, k_reduce / k_reduce_final's sums, the 6 x 6 solve), recomputed step by step from
the trace in numpy.longdouble, and runs longer than the pose-history ring.

test_gpu_loop.py (A5) holds every pt2pt step to 10 x the oracle's own deviation from a
long-double recompute.  Until this file the other three estimators were seen only through
compare_traces (pose within 1e-9 |T| of the oracle's), five orders above what they deliver.
Here every iteration of a run is recomputed from its trace alone:

    kept set   the keys (float distance bits << 32 | query) up to the nkeep-th smallest
    vs, vt     T[it-1] src[kept], tgt[corr_idx[it][kept]]
    pt2pl      r = (vs - vt) . nt, J = [vs x nt, nt], x = solve(J^T J, -J^T r)
    gicp       M = Ct + R Cs0 R^T (R of T[it-1]), A = w^2 M^-1, G = [-[vs]x | I],
               x = solve(sum G^T A G, -sum G^T A (vs - vt)); w = 1, or for cf the mean of the
               two points' lounge confidences
    pose       T[it] = Rz(x2) Ry(x1) Rx(x0), t = x[3:], times T[it-1]

The reference forms W = w (Ct + Cs)^-1/2 and sums (W G)^T (W G); W^T W = w^2 M^-1, so the
system is the same.  The oracle (oracle/refcpu.cpp) keeps the reference's form, and the CPU
tests here measure it against this restatement: that is what proves the identity
numerically, and what the engine's bar is made of.

The bars.  Pose: max(10 x the oracle's largest deviation on the same case, 1e-13 max(1, |T|_F)).
The oracle's own deviation must stay within 1e-13 |T|_F, so no bar is above 1e-12 |T|_F.  The
factor 10 covers the engine's different summation tree and its M^-1 against the oracle's
M^-1/2.  MSE: the mean of K <= n stored float distances summed in any order is within
n 2^-53 of the exact mean, relative; the cf MSE is formed from rounded differences vs - vt and
is held to max(10 x the oracle's deviation, n 2^-53).

Normals come from the side under test: refcpu.estimate_normals for the oracle,
se3icp.estimate_normals (the stage entry) for the engine; 30 neighbours on the target for
pt2pl, 20 on both clouds for gicp and cf (engine.cpp plan_method).  If the stage entry's
normals were not the loop's, a step would miss its bar by many orders.

cf exists only behind the normalization, and its trace is in the normalized frame.  The cf
clouds are built so that the normalization is exact (exact_cf_pair): then the normalized
clouds are the inputs, and the result's T is the last trace row bit for bit.

The runs past the ring (LONG_*): View::hist is a ring of kHist = 256 pose rows indexed
iter % kHist by k_reduce_final, load_hist, k_report_open and the host's result copy, and
prep_settle drops certificates older than the ring.  340 iterations with the switch at 300
put real motion and real searches on ring slots of both generations.
"""
import numpy as np
import pytest

from test_gpu_loop import (B_PARAMS, LD, SUM_ITERS, _apply, _bits, _mse_bar, _pair_b, _rigid, _same_result, _same_trace,
                           assert_exact_cut, nkeep_of, normals_pair, trim_keys)

gpu = pytest.mark.gpu

PHASE_SE3, PHASE_R3 = 1, 2
K_HIST = 256  # common.hpp kHist


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


# =========================================================================== A: the restatement
def solve6_ld(A, b):
    """A x = b in long double by elimination with partial pivoting.  A column whose pivot is
    exactly zero is skipped and leaves that component of x at 0 (the LDLT semantics
    test_pairmath.py states: a zero pivot acts as a pseudo-inverse)."""
    a = np.array(A, dtype=LD)
    y = np.array(b, dtype=LD)
    n = a.shape[0]
    skipped = [False] * n
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if a[p, k] == 0:
            skipped[k] = True
            continue
        if p != k:
            a[[k, p]] = a[[p, k]]
            y[[k, p]] = y[[p, k]]
        f = a[k + 1:, k] / a[k, k]
        a[k + 1:] -= f[:, None] * a[k]
        y[k + 1:] -= f * y[k]
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        if not skipped[k]:
            x[k] = (y[k] - a[k, k + 1:] @ x[k + 1:]) / a[k, k]
    return x


def vec6_to_T_ld(x):
    """TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), t = x[3:] (test_pairmath._vec6)."""
    x = np.asarray(x, dtype=LD)
    cx, sx, cy, sy, cz, sz = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    o, z = LD(1), LD(0)
    Rx = np.array([[o, z, z], [z, cx, -sx], [z, sx, cx]], LD)
    Ry = np.array([[cy, z, sy], [z, o, z], [-sy, z, cy]], LD)
    Rz = np.array([[cz, -sz, z], [sz, cz, z], [z, z, o]], LD)
    T = np.eye(4, dtype=LD)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = x[3:]
    return T


def _skew_ld(v):
    """[v]x of every row of v: (K, 3) -> (K, 3, 3)."""
    z = np.zeros(v.shape[0], LD)
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1), np.stack([v[:, 2], z, -v[:, 0]], -1),
                     np.stack([-v[:, 1], v[:, 0], z], -1)], -2)


def _inv3_batch_ld(m):
    """Cofactor inverses of (K, 3, 3) in long double."""
    c = np.empty_like(m)
    c[:, 0, 0] = m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 2, 1]
    c[:, 0, 1] = m[:, 0, 2] * m[:, 2, 1] - m[:, 0, 1] * m[:, 2, 2]
    c[:, 0, 2] = m[:, 0, 1] * m[:, 1, 2] - m[:, 0, 2] * m[:, 1, 1]
    c[:, 1, 0] = m[:, 1, 2] * m[:, 2, 0] - m[:, 1, 0] * m[:, 2, 2]
    c[:, 1, 1] = m[:, 0, 0] * m[:, 2, 2] - m[:, 0, 2] * m[:, 2, 0]
    c[:, 1, 2] = m[:, 0, 2] * m[:, 1, 0] - m[:, 0, 0] * m[:, 1, 2]
    c[:, 2, 0] = m[:, 1, 0] * m[:, 2, 1] - m[:, 1, 1] * m[:, 2, 0]
    c[:, 2, 1] = m[:, 0, 1] * m[:, 2, 0] - m[:, 0, 0] * m[:, 2, 1]
    c[:, 2, 2] = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 1, 0]
    det = m[:, 0, 0] * c[:, 0, 0] + m[:, 0, 1] * c[:, 1, 0] + m[:, 0, 2] * c[:, 2, 0]
    return c / det[:, None, None]


def _sum0(a):
    """The sum over the first axis, taken along a contiguous last axis (numpy's pairwise sum)."""
    return np.ascontiguousarray(np.moveaxis(a, 0, -1)).sum(-1)


def cov_ld(normals, eps=1e-3):
    """GetRotationFromE1ToX and R diag(eps, 1, 1) R^T of every normal, in long double:
    v = e1 x n, R = I + [v]x + [v]x^2 / (1 + n.x), and R = I where n.x < -0.99 (the comparison
    on the f64 value, as the code under test makes it)."""
    n64 = np.ascontiguousarray(normals, dtype=np.float64).reshape(-1, 3)
    n = n64.astype(LD)
    flat = n64[:, 0] < -0.99
    v = np.stack([np.zeros(n.shape[0], LD), -n[:, 2], n[:, 1]], -1)
    S = _skew_ld(v)
    den = np.where(flat, LD(1), LD(1) + n[:, 0])
    R = np.eye(3, dtype=LD) + S + np.einsum("kab,kbc->kac", S, S) / den[:, None, None]
    R[flat] = np.eye(3, dtype=LD)
    D = np.array([LD(float(eps)), LD(1), LD(1)], LD)
    return np.einsum("kab,b,kcb->kac", R, D, R)


def step_pt2pl_ld(vs, vt, nt):
    """The point-to-plane Gauss-Newton step of K correspondences: the 6-vector x."""
    r = ((vs - vt) * nt).sum(1)
    J = np.concatenate([np.cross(vs, nt), nt], 1)
    H = _sum0(J[:, :, None] * J[:, None, :])
    g = _sum0(J * r[:, None])
    return solve6_ld(H, -g)


def step_gicp_ld(vs, vt, Cs, Ct, w):
    """The GICP step: A = w^2 (Ct + Cs)^-1, G = [-[vs]x | I]."""
    A = _inv3_batch_ld(Ct + Cs) * (w * w)[:, None, None]
    G = np.concatenate([-_skew_ld(vs), np.broadcast_to(np.eye(3, dtype=LD), (vs.shape[0], 3, 3))], 2)
    AG = np.einsum("kab,kbc->kac", A, G)
    H = _sum0(np.einsum("kab,kac->kbc", G, AG))
    g = _sum0(np.einsum("kab,ka->kb", AG, vs - vt))
    return solve6_ld(H, -g)


def lounge_confidence(z):
    """lounge_point_confidence (oracle/refcpu.cpp, ISR.cpp:16-30) of raw depths, in f64 as both
    sides compute it."""
    z = np.asarray(z, dtype=np.float64)
    p1, p2, p3, min_depth = 0.002203, -0.001028, 0.0005351, 0.4
    error = p1 * z * z + p2 * z + p3
    return (p1 * min_depth + p2 * min_depth + p3) / error


def jacobian_step_deviation(est, src, tgt, corr_idx, corr_dist, T_acc, mse, overlap, nt, ns0=None, conf=None,
                            its=None):
    """Every iteration (or those of `its`, 0-based) of a pt2pl / gicp / cf run recomputed from its
    trace alone; the arrays are indexed by iteration, src and tgt are the clouds in the trace's
    frame, nt / ns0 the target / initial source normals, conf = (source, target) confidences
    for cf.  Returns (largest |T[it] - recomputed|_F, largest relative MSE deviation, largest
    |T|_F).  With nothing kept the pose must stay bitwise and the MSE be NaN; with fewer than six
    kept correspondences the system is singular and only the MSE is compared."""
    assert est in ("pt2pl", "gicp", "cf")
    n = src.shape[0]
    k = nkeep_of(n, overlap)
    src_ld, tgt_ld, nt_ld = src.astype(LD), tgt.astype(LD), np.asarray(nt).astype(LD)
    if est != "pt2pl":
        Cs0, Ct0 = cov_ld(ns0), cov_ld(nt)
    dev_T, dev_mse, norm_T = 0.0, 0.0, 1.0
    for it in (range(len(corr_idx)) if its is None else its):
        Tp = np.eye(4) if it == 0 else T_acc[it - 1]
        if k >= n:
            kept = np.arange(n)
        elif k <= 0:
            assert np.array_equal(_bits(T_acc[it]), _bits(Tp)) and np.isnan(mse[it])
            continue
        else:
            keys = trim_keys(corr_dist[it])
            kept = np.nonzero(keys <= np.sort(keys)[k - 1])[0]
            assert kept.shape[0] == k
        Tp = Tp.astype(LD)
        m = corr_idx[it][kept]
        vs = src_ld[kept] @ Tp[:3, :3].T + Tp[:3, 3]
        vt = tgt_ld[m]
        if est == "pt2pl":
            x = step_pt2pl_ld(vs, vt, nt_ld[m])
        else:
            R = Tp[:3, :3]
            Cs = np.einsum("ab,kbc,dc->kad", R, Cs0[kept], R)
            w = np.ones(kept.shape[0], LD) if est == "gicp" else (conf[0][kept].astype(LD) + conf[1][m].astype(LD)) / LD(2)
            x = step_gicp_ld(vs, vt, Cs, Ct0[m], w)
        if est == "cf":
            want_mse = np.sqrt(((vs - vt) ** 2).sum(1)).sum() / LD(kept.shape[0])
        else:
            want_mse = corr_dist[it][kept].astype(LD).sum() / LD(kept.shape[0])
        if kept.shape[0] >= 6:  # (fewer cannot determine six unknowns: see the one-correspondence test)
            want_T = vec6_to_T_ld(x) @ Tp
            dev_T = max(dev_T, float(np.sqrt(((T_acc[it].astype(LD) - want_T) ** 2).sum())))
            norm_T = max(norm_T, float(np.linalg.norm(T_acc[it])))
        if want_mse > 0:
            dev_mse = max(dev_mse, float(abs(LD(mse[it]) - want_mse) / want_mse))
        else:
            assert mse[it] == 0.0
    return dev_T, dev_mse, norm_T


def r3_distance_ulps(src, tgt, corr_idx, corr_dist, T_acc, its):
    """The largest distance, in float ulps, between the stored corr_dist[it][i] and
    float32(|T[it-1] src_i - tgt[corr_idx[it][i]]|) over the iterations `its` (R3 phase)."""
    src_ld, tgt_ld = src.astype(LD), tgt.astype(LD)
    worst = 0
    for it in its:
        Tp = (np.eye(4) if it == 0 else T_acc[it - 1]).astype(LD)
        d = np.sqrt(((src_ld @ Tp[:3, :3].T + Tp[:3, 3] - tgt_ld[corr_idx[it]]) ** 2).sum(1)).astype(np.float32)
        worst = max(worst, int(np.abs(d.view(np.int32).astype(np.int64) -
                                      np.ascontiguousarray(corr_dist[it]).view(np.int32).astype(np.int64)).max()))
    return worst


def _mul4(a, b):
    """The oracle's 4 x 4 product (refcpu.cpp mul: the four terms added left to right, no FMA)."""
    return ((a[:, 0, None] * b[0] + a[:, 1, None] * b[1]) + a[:, 2, None] * b[2]) + a[:, 3, None] * b[3]


def oracle_poses(ref):
    """The oracle's accumulated pose after every iteration, as it forms it: T <- Ti T."""
    out, T = [], np.eye(4)
    for it in range(ref["num_iterations"]):
        T = _mul4(ref["Ti"][it], T)
        out.append(T)
    return out


# --------------------------------------------------------------------------- A1 - A3 on the CPU
def test_solve6_ld_against_numpy():
    rng = np.random.default_rng(3)
    for _ in range(20):
        J = rng.normal(size=(40, 6))
        A, b = J.T @ J, rng.normal(size=6)
        x = solve6_ld(A, b)
        want = np.linalg.solve(A, b)
        # numpy's f64 solve carries cond(A) eps; the long-double solve a thousandth of that
        assert float(np.abs(x - want).max()) <= 10 * np.linalg.cond(A) * 2.0 ** -52 * np.abs(want).max()
        assert float(np.abs(A.astype(LD) @ x - b).max()) <= 1e-17 * np.abs(A).max() * float(np.abs(x).max()) * 6
    # a zero pivot leaves its component at 0; the all-zero system gives 0
    A = np.diag([2.0, 3.0, 4.0, 5.0, 6.0, 0.0])
    b = np.array([1.0, -1.0, 2.0, 0.5, -0.5, 0.0])
    want = np.zeros(6)
    want[:5] = b[:5] / np.diag(A)[:5]
    assert np.array_equal(solve6_ld(A, b).astype(np.float64), want)
    assert not solve6_ld(np.zeros((6, 6)), np.zeros(6)).any()
    # partial pivoting: a zero in the leading position is no zero pivot
    P = np.eye(6)[[1, 0, 2, 3, 4, 5]]
    assert np.array_equal(solve6_ld(P, np.arange(6.0)).astype(np.float64), P.T @ np.arange(6.0))


def test_vec6_to_T_ld_against_the_f64_restatement():
    from test_pairmath import _vec6
    rng = np.random.default_rng(4)
    for _ in range(20):
        x = np.concatenate([rng.uniform(-np.pi, np.pi, 3), rng.uniform(-5, 5, 3)])
        T = vec6_to_T_ld(x)
        assert float(np.abs(T - _vec6(x)).max()) <= 1e-15
        assert float(np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max()) <= 1e-18
    assert np.array_equal(vec6_to_T_ld(np.zeros(6)).astype(np.float64), np.eye(4))


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def test_cov_ld_against_the_oracle(refcpu):
    """1,000 random unit normals and 200 within 8 degrees of -e1 (both sides of the branch)."""
    rng = np.random.default_rng(6)
    near = np.stack([-np.ones(200), rng.uniform(-0.14, 0.14, 200), rng.uniform(-0.14, 0.14, 200)], 1)
    near /= np.linalg.norm(near, axis=1)[:, None]
    nrm = np.concatenate([unit_normals(1000, 5), near])
    taken = int((nrm[:, 0] < -0.99).sum())
    assert 20 <= taken <= 200 and int((near[:, 0] >= -0.99).sum()) >= 20
    dev = float(np.abs(cov_ld(nrm) - refcpu.gicp_covariances(nrm)).max())
    print(f"[steps] cov_ld against the oracle: {dev:.2e} over {len(nrm)} normals, {taken} on the R = I branch")
    assert dev <= 1e-15
    assert np.array_equal(cov_ld(nrm[nrm[:, 0] < -0.99]).astype(np.float64),
                          np.broadcast_to(np.diag([1e-3, 1.0, 1.0]), (taken, 3, 3)))


# =========================================================================== the cases
STEP_SIZES = [1, 255, 256, 257, 32256, 32257, 36864, 36865]  # 1 | 2 and 126 | 127 | 144 | 145 blocks of k_reduce
STEP_OVERLAPS = [1.0, 0.7]
STEP_METHODS = ["pt2pl", "gicp"]
POSE_CONDITION = 1e-13   # the oracle's own deviation over |T|_F: keeps every engine bar <= 1e-12 |T|_F

_CASES = {}


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _normals_for(est, side, pair):
    """(target normals, initial source normals or None) from `side`.estimate_normals."""
    src, tgt = pair
    if est == "pt2pl":
        return side.estimate_normals(tgt, 30), None
    return side.estimate_normals(tgt, 20), side.estimate_normals(src, 20)


def _run_oracle(refcpu, pair, rkind, variant, params, rows):
    return refcpu.register(pair[0], pair[1], rkind, variant, refcpu.default_params(**params), trace_iters=rows)


def oracle_icp_case(refcpu, key, pair, variant, params, rows):
    """One run_icp oracle run, its deviation from the recompute, and what the engine's test
    needs of it (not the trace: 37k points x rows), once per key."""
    if key not in _CASES:
        ref = _run_oracle(refcpu, pair, refcpu.RUN_ICP, variant, params, rows)
        n_it = ref["num_iterations"]
        assert n_it <= rows
        nt, ns0 = _normals_for(variant, refcpu, pair)
        dev = jacobian_step_deviation(variant, pair[0], pair[1], ref["corr_idx"][:n_it], ref["corr_dist"][:n_it],
                                      oracle_poses(ref), ref["mse"][:n_it], params["estimated_overlap"], nt, ns0)
        _CASES[key] = dict(num_iterations=n_it, first_idx=ref["corr_idx"][0].copy(), T=ref["T"], dev=dev,
                           ns0=ns0, nt=nt)
    return _CASES[key]


def _step_params(overlap):
    return dict(estimated_overlap=overlap, max_num_iterations=SUM_ITERS, mse=0.0)


def _report_oracle(what, case, n):
    dev_T, dev_mse, norm_T = case["dev"]
    print(f"[steps] oracle {what}: {case['num_iterations']} iterations, |T - T_ld|_F {dev_T:.2e} "
          f"(|T|_F {norm_T:.3g}), mse {dev_mse:.2e} relative")
    assert dev_T <= POSE_CONDITION * norm_T, (what, dev_T, norm_T)
    return dev_T, dev_mse, norm_T


def engine_icp_case(mod, refcpu, parity_record, name, what, pair, variant, params, want, blocks):
    """test_jacobian_step_recomputed_from_the_trace for one run_icp case; returns the trace."""
    n, overlap = pair[0].shape[0], params["estimated_overlap"]
    gp = mod.default_params(**params)
    res, gtr = mod.register_batch_traced([pair], variant, gp, pair=0, max_iters=want["num_iterations"] + 2)
    g = res[0]
    assert g.status == 0 and g.num_iterations == want["num_iterations"] == len(gtr["phase"])
    assert_exact_cut(gtr, n, overlap)
    assert np.array_equal(gtr["corr_idx"][0], want["first_idx"])
    nt, ns0 = _normals_for(variant, mod, pair)
    dev_T, dev_mse, norm_T = jacobian_step_deviation(variant, pair[0], pair[1], gtr["corr_idx"], gtr["corr_dist"], gtr["T"],
                                                     gtr["mse"], overlap, nt, ns0)
    ref_T, ref_mse, _ = want["dev"]
    bar = max(10 * ref_T, POSE_CONDITION * norm_T)
    print(f"[steps] engine {what}: |T - T_ld|_F {dev_T:.2e} (oracle {ref_T:.2e}, bar {bar:.2e}), mse {dev_mse:.2e} "
          f"(oracle {ref_mse:.2e}, bar {_mse_bar(n):.2e})")
    parity_record(name, blocks=blocks, iterations=int(g.num_iterations), oracle_pose_dev=ref_T, engine_pose_dev=dev_T,
                  pose_bar=bar, oracle_mse_dev=ref_mse, engine_mse_dev=dev_mse, mse_bar=_mse_bar(n))
    assert bar <= 1e-12 * norm_T
    assert dev_T <= bar, (what, dev_T, bar)
    assert dev_mse <= _mse_bar(n), (what, dev_mse)
    plain = mod.register_batch([pair], variant, gp)[0]
    assert _same_result(plain, g), (what, "untraced run differs")
    return g, gtr


# --------------------------------------------------------------------------- B1: reduction edges
def _b1(refcpu, variant, n, overlap):
    return oracle_icp_case(refcpu, ("b1", variant, n, overlap), normals_pair(n), variant, _step_params(overlap),
                           SUM_ITERS + 2)


@pytest.mark.parametrize("overlap", STEP_OVERLAPS)
@pytest.mark.parametrize("n", STEP_SIZES)
@pytest.mark.parametrize("variant", STEP_METHODS)
def test_oracle_jacobian_step_deviation(refcpu, variant, n, overlap):
    """The oracle's own pt2pl / gicp steps (f64, W = M^-1/2, covariances rotated step by step, 64
    chunks summed in order) against the long-double recompute of its own trace: SUM_ITERS
    iterations, pose within 1e-13 |T|_F, MSE within the bound of any summation order."""
    case = _b1(refcpu, variant, n, overlap)
    assert case["num_iterations"] == SUM_ITERS
    _, dev_mse, _ = _report_oracle(f"{variant} n {n} overlap {overlap}", case, n)
    assert dev_mse <= _mse_bar(n)


@gpu
@pytest.mark.parametrize("overlap", STEP_OVERLAPS)
@pytest.mark.parametrize("n", STEP_SIZES)
@pytest.mark.parametrize("variant", STEP_METHODS)
def test_jacobian_step_recomputed_from_the_trace(se3icp_mod, refcpu, parity_record, variant, n, overlap):
    """corr_terms' pt2pl and GICP branches, k_reduce's 27 sums, k_reduce_final's chains and the
    6 x 6 solve at the reduction's structural sizes, raw coordinates (|p| up to 60): every
    iteration's pose within max(10 x the oracle's deviation, 1e-13 max(1, |T|_F)) of the
    long-double recompute of the engine's own trace, with the stage entry's normals."""
    pair = normals_pair(n)
    g, gtr = engine_icp_case(se3icp_mod, refcpu, parity_record, f"loop: {variant} step n={n} overlap={overlap}",
                             f"{variant} n {n} overlap {overlap}", pair, variant, _step_params(overlap),
                             _b1(refcpu, variant, n, overlap), (n + 255) // 256)
    _GPU_RUNS[(variant, n, overlap)] = (g, gtr)


_GPU_RUNS = {}


def test_one_correspondence_leaves_the_step_undetermined(refcpu):
    """n = 1 at overlap 1.0 keeps one correspondence: J^T J has rank 1 (pt2pl) or 3 (gicp) of 6,
    the pivots behind it are the rounding of zero, and the step is whatever those roundings
    make it on either side (the oracle lands 24 and 0.64 |.|_F away from the long-double
    solve).  jacobian_step_deviation therefore compares the pose only where at least six
    correspondences are kept, and this test states why: the one-point system, formed in long
    double, has singular values past its rank below 1e-13 of the largest."""
    src = normals_pair(1)[0]
    for variant in STEP_METHODS:
        case = _b1(refcpu, variant, 1, 1.0)
        assert case["num_iterations"] == SUM_ITERS and np.isfinite(case["T"]).all()
        vs, m = src.astype(LD), case["first_idx"]
        if variant == "pt2pl":
            J = np.concatenate([np.cross(vs, case["nt"].astype(LD)[m]), case["nt"].astype(LD)[m]], 1)
            H = J.T @ J
        else:
            G = np.concatenate([-_skew_ld(vs), np.eye(3, dtype=LD)[None]], 2)[0]
            H = G.T @ _inv3_batch_ld(cov_ld(case["ns0"]) + cov_ld(case["nt"])[m])[0] @ G
        sv = np.linalg.svd(H.astype(np.float64), compute_uv=False)
        rank = 1 if variant == "pt2pl" else 3
        assert sv[rank] <= 1e-13 * sv[0] < 1e-3 * sv[rank - 1], (variant, sv)


# --------------------------------------------------------------------------- B2: cf, exact normalization
CF_HALVES = [128, 129, 16129, 18433]  # mirrored: 256 | 258 | 32,258 | 36,866 source points = 1 | 2 | 127 | 145 blocks
CF_PARAMS = dict(estimated_overlap=0.8, max_num_se3_iterations=3, max_num_iterations=8, mse=0.0,
                 scale_preprocessing=4.0)
CF_GRID = 2.0 ** -10
_CF_PAIRS = {}


def exact_cf_pair(bunny_unique, half):
    """A pair whose normalization is exact.  Every coordinate is a multiple of 2^-10 below 4,
    so sums of 2^15 of them are exact in f64; every cloud is concat(Q, -Q), so its centroid is
    exactly 0 in any summation order; the target also carries (+-4, 0, 0) and every other
    point lies within radius 3.5, so the largest radius is exactly 4 and, with
    scale_preprocessing = 4, scaling_factor = 4 * (1 / 4) = 1.  Q: `half` samples of the bunny
    (centred, radius 3; with replacement beyond its size) moved by a small rotation plus noise
    for the source, 2,000 samples for the target."""
    if half not in _CF_PAIRS:
        rng = np.random.default_rng(4100 + half)
        b = bunny_unique - bunny_unique.mean(0)
        b *= 3.0 / np.linalg.norm(b, axis=1).max()
        qt = b[rng.choice(len(b), 2000, replace=False)]
        qs = b[rng.choice(len(b), half, replace=half > len(b) // 2)]
        qs = _apply(_rigid(0.05, -0.04, 0.06, 0.0), qs) + rng.normal(0.0, 0.002, qs.shape)
        qs, qt = np.round(qs / CF_GRID) * CF_GRID, np.round(qt / CF_GRID) * CF_GRID
        src = np.ascontiguousarray(np.concatenate([qs, -qs]))
        tgt = np.ascontiguousarray(np.concatenate([qt, -qt, [[4.0, 0.0, 0.0], [-4.0, 0.0, 0.0]]]))
        for c in (src, tgt):
            assert np.array_equal(np.round(c / CF_GRID) * CF_GRID, c)
            assert not np.cumsum(c, axis=0)[-1].any() and not c.sum(0).any()
        assert np.linalg.norm(src, axis=1).max() < 3.5 and np.linalg.norm(tgt[:-2], axis=1).max() < 3.5
        assert np.sqrt((tgt * tgt).sum(1)).max() == 4.0
        _CF_PAIRS[half] = _freeze(src, tgt)
    return _CF_PAIRS[half]


def _cf_conf(pair):
    return lounge_confidence(pair[0][:, 2]), lounge_confidence(pair[1][:, 2])


def _cf_deviation(pair, side, corr_idx, corr_dist, T_acc, mse):
    nt, ns0 = _normals_for("cf", side, pair)
    return jacobian_step_deviation("cf", pair[0], pair[1], corr_idx, corr_dist, T_acc, mse, CF_PARAMS["estimated_overlap"],
                                   nt, ns0, _cf_conf(pair))


def _oracle_cf(refcpu, bunny_unique, half):
    key = ("cf", half)
    if key not in _CASES:
        pair = exact_cf_pair(bunny_unique, half)
        ref = _run_oracle(refcpu, pair, refcpu.RUN_SE3_ICP_CF, "gicp", CF_PARAMS, 10)
        n_it = ref["num_iterations"]
        poses = oracle_poses(ref)
        # the three facts without which the case proves nothing
        assert ref["scaling_factor"] == 1.0
        assert np.array_equal(_bits(ref["T"]), _bits(poses[-1] + 0.0))
        dev = _cf_deviation(pair, refcpu, ref["corr_idx"][:n_it], ref["corr_dist"][:n_it], poses, ref["mse"][:n_it])
        pure = ref["num_pure_se3_iterations"]
        ulps = r3_distance_ulps(pair[0], pair[1], ref["corr_idx"], ref["corr_dist"], poses, range(pure, n_it))
        _CASES[key] = dict(num_iterations=n_it, pure=pure, first_idx=ref["corr_idx"][0].copy(), T=ref["T"], dev=dev,
                           r3_ulps=ulps)
    return _CASES[key]


@pytest.mark.parametrize("half", CF_HALVES)
def test_oracle_cf_step_deviation(refcpu, bunny_unique, half):
    """The oracle's confidence-weighted GICP (W = w M^-1/2, Euclidean MSE) on the exactly
    normalized pair: 8 iterations, 3 of them in the SE(3) phase, scaling_factor 1.0, the result
    the last trace row bitwise; pose within 1e-13 |T|_F of the recompute.  Its relative MSE
    deviation (the rounding of vs - vt and of the sum) is recorded: it sets the engine's bar."""
    case = _oracle_cf(refcpu, bunny_unique, half)
    assert (case["num_iterations"], case["pure"]) == (8, 3)
    _, dev_mse, _ = _report_oracle(f"cf n {2 * half}", case, 2 * half)
    print(f"[steps] oracle cf n {2 * half}: mse deviation {dev_mse:.2e} relative, R3 distances within {case['r3_ulps']} ulp")
    assert case["r3_ulps"] <= 1
    assert dev_mse <= 1e-13  # a sanity ceiling; the engine's bar is 10 x the figure itself


@gpu
@pytest.mark.parametrize("half", CF_HALVES)
def test_cf_step_recomputed_from_the_trace(se3icp_mod, refcpu, bunny_unique, parity_record, half):
    """corr_terms' cf branch (A = w^2 M^-1, the Euclidean MSE) in both phases at 1, 2, 127 and
    145 blocks, on a pair whose normalization is exact."""
    pair = exact_cf_pair(bunny_unique, half)
    n, overlap = 2 * half, CF_PARAMS["estimated_overlap"]
    want = _oracle_cf(refcpu, bunny_unique, half)
    gp = se3icp_mod.default_params(**CF_PARAMS)
    res, gtr = se3icp_mod.register_batch_traced([pair], "se3_gicp_with_cf", gp, pair=0, max_iters=10)
    g = res[0]
    assert g.status == 0 and (g.num_iterations, g.num_pure_se3_iterations) == (want["num_iterations"], want["pure"])
    assert gtr["phase"].tolist() == [PHASE_SE3] * want["pure"] + [PHASE_R3] * (want["num_iterations"] - want["pure"])
    assert g.scaling_factor == 1.0
    assert np.array_equal(_bits(g.T), _bits(gtr["T"][-1] + 0.0))
    assert_exact_cut(gtr, n, overlap)
    assert np.array_equal(gtr["corr_idx"][0], want["first_idx"])
    ulps = r3_distance_ulps(pair[0], pair[1], gtr["corr_idx"], gtr["corr_dist"], gtr["T"],
                            range(want["pure"], want["num_iterations"]))
    assert ulps <= 1, ulps
    dev_T, dev_mse, norm_T = _cf_deviation(pair, se3icp_mod, gtr["corr_idx"], gtr["corr_dist"], gtr["T"], gtr["mse"])
    ref_T, ref_mse, _ = want["dev"]
    bar, mse_bar = max(10 * ref_T, POSE_CONDITION * norm_T), max(10 * ref_mse, _mse_bar(n))
    print(f"[steps] engine cf n {n}: |T - T_ld|_F {dev_T:.2e} (oracle {ref_T:.2e}, bar {bar:.2e}), mse {dev_mse:.2e} "
          f"(oracle {ref_mse:.2e}, bar {mse_bar:.2e})")
    parity_record(f"loop: cf step n={n} overlap={overlap}", blocks=(n + 255) // 256, iterations=int(g.num_iterations),
                  oracle_pose_dev=ref_T, engine_pose_dev=dev_T, pose_bar=bar, oracle_mse_dev=ref_mse,
                  engine_mse_dev=dev_mse, mse_bar=mse_bar, r3_distance_ulps=ulps)
    assert bar <= 1e-12 * norm_T
    assert dev_T <= bar, (n, dev_T, bar)
    assert dev_mse <= mse_bar, (n, dev_mse, mse_bar)
    assert _same_result(se3icp_mod.register_batch([pair], "se3_gicp_with_cf", gp)[0], g)


# --------------------------------------------------------------------------- B3: far from the identity
FAR_ITERATIONS = {"gicp": 24, "pt2pl": 47}


def _far(refcpu, bunny_unique, variant):
    return oracle_icp_case(refcpu, ("far", variant), _pair_b(bunny_unique), variant, B_PARAMS, 160)


@pytest.mark.parametrize("variant", list(FAR_ITERATIONS))
def test_oracle_step_deviation_far_from_the_identity(refcpu, bunny_unique, variant):
    """The bunny pair (45 degrees of initial error, |T|_F up to 9): every one of the oracle's
    24 (gicp) and 47 (pt2pl) iterations within 1e-13 |T|_F of the recompute, which rotates the
    initial covariances by the accumulated pose where the oracle rotates them step by step."""
    case = _far(refcpu, bunny_unique, variant)
    assert case["num_iterations"] == FAR_ITERATIONS[variant]
    _, dev_mse, _ = _report_oracle(f"{variant} bunny", case, 3544)
    assert dev_mse <= _mse_bar(3544)


@gpu
@pytest.mark.parametrize("variant", list(FAR_ITERATIONS))
def test_jacobian_step_far_from_the_identity(se3icp_mod, refcpu, bunny_unique, parity_record, variant):
    """Cs = R Cs0 R^T from the accumulated pose (corr_terms), and the Jacobian about the origin
    with a large lever arm, over a whole run from 45 degrees out."""
    engine_icp_case(se3icp_mod, refcpu, parity_record, f"loop: {variant} step n=3544 overlap=0.7 (bunny, 45 degrees)",
                    f"{variant} bunny", _pair_b(bunny_unique), variant, B_PARAMS, _far(refcpu, bunny_unique, variant), 14)


# --------------------------------------------------------------------------- B4: one mixed-size batch
BATCH_SIZES = [255, 257, 32257]


@gpu
def test_mixed_size_gicp_batch(se3icp_mod, refcpu, parity_record):
    """Three gicp pairs of 1, 2 and 127 blocks in one batch, traced once per pair: each trace and
    result bitwise the pair's alone, and each within its step bar."""
    overlap = 0.7
    pairs = [normals_pair(n) for n in BATCH_SIZES]
    gp = se3icp_mod.default_params(**_step_params(overlap))
    alone = []
    for n, pair in zip(BATCH_SIZES, pairs):
        if ("gicp", n, overlap) not in _GPU_RUNS:
            res, gtr = se3icp_mod.register_batch_traced([pair], "gicp", gp, pair=0, max_iters=SUM_ITERS + 2)
            _GPU_RUNS[("gicp", n, overlap)] = (res[0], gtr)
        alone.append(_GPU_RUNS[("gicp", n, overlap)])
    for k, (n, pair) in enumerate(zip(BATCH_SIZES, pairs)):
        res, gtr = se3icp_mod.register_batch_traced(pairs, "gicp", gp, pair=k, max_iters=SUM_ITERS + 2)
        assert _same_trace(gtr, alone[k][1]), (n, [key for key in gtr if not np.array_equal(_bits(gtr[key]),
                                                                                         _bits(alone[k][1][key]))])
        for j in range(len(pairs)):
            assert _same_result(res[j], alone[j][0]), (n, BATCH_SIZES[j])
        want = _b1(refcpu, "gicp", n, overlap)
        nt, ns0 = _normals_for("gicp", se3icp_mod, pair)
        dev_T, dev_mse, norm_T = jacobian_step_deviation("gicp", pair[0], pair[1], gtr["corr_idx"], gtr["corr_dist"],
                                                         gtr["T"], gtr["mse"], overlap, nt, ns0)
        bar = max(10 * want["dev"][0], POSE_CONDITION * norm_T)
        parity_record(f"loop: gicp step batch of {len(pairs)} n={n} overlap={overlap}", blocks=(n + 255) // 256,
                      oracle_pose_dev=want["dev"][0], engine_pose_dev=dev_T, pose_bar=bar, oracle_mse_dev=want["dev"][1],
                      engine_mse_dev=dev_mse, mse_bar=_mse_bar(n))
        assert dev_T <= bar and dev_mse <= _mse_bar(n), (n, dev_T, bar, dev_mse)


# =========================================================================== D: runs past the ring
# The bunny pair with the SE(3) phase capped at 300 iterations and the run at 340, and both
# stopping tests switched off (`rel < sf * mse` and `change < mse_switch_error` are strict, so
# 0 never fires).  On the oracle the pose is still from iteration ~100 to 300 (steps ~1e-17):
# every settled certificate ages out of the ring at it - ci = 256.  The switch at 301 moves the
# pose again and changes thousands of correspondences while the ring holds rows of both
# generations, and the certificates of the first phase must be void (ci >= phase_start).
LONG_PARAMS = dict(B_PARAMS, max_num_se3_iterations=300, max_num_iterations=340, mse=0.0, mse_switch_error=0.0)
LONG_ITERS, LONG_SE3 = 340, 300
assert LONG_SE3 > K_HIST  # the switch comes after the ring has wrapped
LONG_ROWS = 344
LONG_STEP_ITS = range(298, 312)  # iterations 299 ... 312, 0-based
LONG_METHODS = ["pt2pl", "gicp"]
_LONG = {}


def normalized_pair(src, tgt, scale_preprocessing):
    """The normalization of run_se3_* as the oracle (se3_setup) and the engine compute it in f64:
    centroids by sums in point order, the larger of the two largest radii, s = scale * (1 / r),
    p' = (p - c) * s.  Returns (src', tgt', s)."""
    out, r = [], []
    for c in (src, tgt):
        centre = np.cumsum(c, axis=0)[-1] / float(c.shape[0])  # (cumsum adds in order)
        d = c - centre
        r.append(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
        out.append(d)
    s = scale_preprocessing * (1.0 / max(r))
    return np.ascontiguousarray(out[0] * s), np.ascontiguousarray(out[1] * s), s


def _long_frame(refcpu, bunny_unique):
    if "frame" not in _LONG:
        src, tgt = _pair_b(bunny_unique)
        s_n, t_n, s = normalized_pair(src, tgt, refcpu.default_params().scale_preprocessing)
        _LONG["frame"] = _freeze(s_n, t_n) + (s,)
    return _LONG["frame"]


def _long_deviation(side, frame, variant, corr_idx, corr_dist, T_acc, mse):
    pair = frame[:2]
    nt, ns0 = _normals_for(variant, side, pair)
    return jacobian_step_deviation(variant, pair[0], pair[1], corr_idx, corr_dist, T_acc, mse, LONG_PARAMS["estimated_overlap"],
                                   nt, ns0, its=LONG_STEP_ITS)


def _oracle_long(refcpu, bunny_unique, variant):
    if variant not in _LONG:
        pair = _pair_b(bunny_unique)
        ref = refcpu.register(pair[0], pair[1], refcpu.RUN_SE3_ICP, variant, refcpu.default_params(**LONG_PARAMS),
                              trace_iters=LONG_ROWS, trace_margins=True)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        frame = _long_frame(refcpu, bunny_unique)
        n_it = ref["num_iterations"]
        dev = _long_deviation(refcpu, frame, variant, ref["corr_idx"][:n_it], ref["corr_dist"][:n_it], oracle_poses(ref),
                              ref["mse"][:n_it]) if n_it == LONG_ITERS else None
        _LONG[variant] = (ref, dev)
    return _LONG[variant]


@pytest.mark.parametrize("variant", LONG_METHODS)
def test_oracle_long_run_facts(refcpu, bunny_unique, variant):
    """What makes the long run a test of the ring, asserted on the oracle: 340 iterations, 300
    of them SE(3); no motion over iterations 150 ... 300; the switch moves the pose by more than
    1e-4 and changes more than 1,000 correspondences.  And the condition of the step bar on
    iterations 299 ... 312, in the normalized frame restated by normalized_pair (the scaling
    factor bitwise the oracle's)."""
    ref, dev = _oracle_long(refcpu, bunny_unique, variant)
    assert (ref["num_iterations"], ref["num_pure_se3_iterations"]) == (LONG_ITERS, LONG_SE3)
    step = [float(np.linalg.norm(ref["Ti"][it] - np.eye(4))) for it in range(LONG_ITERS)]
    changed = int((ref["corr_idx"][LONG_SE3] != ref["corr_idx"][LONG_SE3 - 1]).sum())
    print(f"[steps] oracle long se3_{variant}: largest step over 150..300 {max(step[149:LONG_SE3]):.2e}, step at 301 "
          f"{step[LONG_SE3]:.2e}, {changed} correspondences changed at the switch, steps 302..312 "
          f"{min(step[LONG_SE3 + 1:312]):.1e} .. {max(step[LONG_SE3 + 1:312]):.1e}")
    assert max(step[149:LONG_SE3]) < 1e-12
    assert step[LONG_SE3] > 1e-4
    assert changed > 1000
    assert ref["scaling_factor"] == _long_frame(refcpu, bunny_unique)[2]
    dev_T, dev_mse, norm_T = dev
    print(f"[steps] oracle long se3_{variant}: iterations 299..312 |T - T_ld|_F {dev_T:.2e} (|T|_F {norm_T:.3g}), "
          f"mse {dev_mse:.2e} relative")
    assert dev_T <= POSE_CONDITION * norm_T and dev_mse <= _mse_bar(3544)


def _engine_long(mod, bunny_unique, variant):
    key = ("gpu", variant)
    if key not in _LONG:
        pair = _pair_b(bunny_unique)
        res, gtr = mod.register_batch_traced([pair], "se3_" + variant, mod.default_params(**LONG_PARAMS), pair=0,
                                             max_iters=LONG_ROWS)
        _LONG[key] = (res[0], gtr)
    return _LONG[key]


@gpu
@pytest.mark.parametrize("variant", LONG_METHODS)
def test_long_run_trace_past_the_ring(se3icp_mod, refcpu, bunny_unique, parity_record, variant):
    """340 traced iterations (lag = 0) against the oracle's, row by row: no unexcused index
    difference, the exact cut, the phases; the untraced run (look-ahead, lag = 1) bitwise equal;
    the step bar on iterations 299 ... 312, across the switch."""
    from test_gpu_trace import compare_traces
    ref, want = _oracle_long(refcpu, bunny_unique, variant)
    g, gtr = _engine_long(se3icp_mod, bunny_unique, variant)
    pair = _pair_b(bunny_unique)
    assert g.status == 0 and (g.num_iterations, g.num_pure_se3_iterations) == (LONG_ITERS, LONG_SE3)
    assert gtr["phase"].tolist() == [PHASE_SE3] * LONG_SE3 + [PHASE_R3] * (LONG_ITERS - LONG_SE3)
    tot = compare_traces(gtr, ref, LONG_PARAMS["estimated_overlap"], f"long se3_{variant}")
    assert_exact_cut(gtr, pair[0].shape[0], LONG_PARAMS["estimated_overlap"])
    frame = _long_frame(refcpu, bunny_unique)
    assert g.scaling_factor == frame[2]
    assert r3_distance_ulps(frame[0], frame[1], gtr["corr_idx"], gtr["corr_dist"], gtr["T"], range(LONG_SE3, 312)) <= 1
    dev_T, dev_mse, norm_T = _long_deviation(se3icp_mod, frame, variant, gtr["corr_idx"], gtr["corr_dist"], gtr["T"],
                                             gtr["mse"])
    bar = max(10 * want[0], POSE_CONDITION * norm_T)
    print(f"[steps] engine long se3_{variant}: iterations 299..312 |T - T_ld|_F {dev_T:.2e} (oracle {want[0]:.2e}, bar "
          f"{bar:.2e}), mse {dev_mse:.2e}")
    parity_record(f"loop: long run se3_{variant} n=3544 overlap=0.7", iterations=int(g.num_iterations),
                  pure_se3_iterations=int(g.num_pure_se3_iterations), idx_diff=tot["idx_diff"], dist_ulp1=tot["dist_ulp1"],
                  kept_swaps=tot["kept_swaps"], max_pose_diff=tot["max_pose_diff"], blocks=14, oracle_pose_dev=want[0],
                  engine_pose_dev=dev_T, pose_bar=bar, oracle_mse_dev=want[1], engine_mse_dev=dev_mse, mse_bar=_mse_bar(3544))
    assert bar <= 1e-12 * norm_T
    assert dev_T <= bar and dev_mse <= _mse_bar(3544), (variant, dev_T, bar, dev_mse)
    plain = se3icp_mod.register_batch([pair], "se3_" + variant, se3icp_mod.default_params(**LONG_PARAMS))[0]
    assert _same_result(plain, g), (variant, "untraced run differs", plain.num_iterations, g.num_iterations)


@gpu
@pytest.mark.parametrize("variant", LONG_METHODS)
def test_long_run_report_and_sweep(se3icp_mod, bunny_unique, variant):
    """k_report_open reads the final pose at it % kHist with it = 341: the report's result is
    bitwise the plain one, and its final matches are the nearest neighbours at the final pose.
    A sweep with max_num_se3_iterations 10 and 300 in one group (one variant in the R3 phase
    while the other is still in the SE(3) phase, both past the ring) equals the two calls."""
    from test_gpu_report import nearest
    g, _ = _engine_long(se3icp_mod, bunny_unique, variant)
    src, tgt = _pair_b(bunny_unique)
    prm = se3icp_mod.default_params(**LONG_PARAMS)
    res, rep = se3icp_mod.register_batch_report([(src, tgt)], "se3_" + variant, prm, per_point=True)
    assert _same_result(res[0], g)
    q = src @ g.T[:3, :3].T + g.T[:3, 3]
    j, d, second = nearest(q, tgt, brute=True)
    tie = (second - d) <= 1e-9 * second
    assert np.array_equal(rep[0].corr_idx[~tie], j[~tie].astype(np.int32)) and int(tie.sum()) <= 3
    assert rep[0].fitness == 1.0 and rep[0].n_inliers == src.shape[0]
    short = se3icp_mod.default_params(**dict(LONG_PARAMS, max_num_se3_iterations=10))
    both = se3icp_mod.register_sweep([(src, tgt)], "se3_" + variant, [short, prm], max_group=2)
    alone = se3icp_mod.register_batch([(src, tgt)], "se3_" + variant, short)[0]
    assert (alone.num_iterations, alone.num_pure_se3_iterations) == (LONG_ITERS, 10)
    assert _same_result(both[0][0], alone) and _same_result(both[1][0], g)
