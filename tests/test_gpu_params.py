"""GPU parity over the reference's parameter sweep, not only its defaults.

Every other GPU parity test runs with alpha_rot = 3, beta_transl = 1, scale_preprocessing = 3
and max_num_iterations = 150, where several code paths equal a wrong version of themselves:
with beta = 1 an element's translation rows are the point (so the cf branches of
store_frame_rows / target12 / match_anchor are no-ops), with alpha = 3 a constant in place
of alpha^2 in the f32 certificate (k_nn.hip prep_settle) goes unnoticed, nothing compares
scaling_factor, and the host loop never meets a binding iteration cap.  The reference's own
drivers sweep these public fields (makeHybridLGrid() of examples/benchmark_*.cpp: alpha_rot
from 0 to 1000), so this file runs the engine against the oracle across them, on inputs of
3.5k - 4.5k points:

  B  datasets.bunny_pair(bunny_unique, seed=2, subsample=0.1): 3544 / 3563 noisy points
  R  datasets.rgbd_pairs(1, seed=5, stride=8)[0][0]: 4413 / 4397 points
  F  the golden fixture clouds: 4167 noise-free points, 188 groups of duplicates

Every traced case asserts: iteration counts of both phases equal the oracle's;
test_gpu_trace.compare_traces with its bars unchanged (per-iteration pose and MSE 1e-9
relative, float distances <= 1 ulp); no index difference at all; final pose within 1e-5
Frobenius; scaling_factor within 1e-10 relative (exactly 1.0 for run_icp).

* idx_diff == 0: compare_traces excuses an index difference only where the oracle's own two
  best targets are a rounding-level near-tie.  The oracle alone, on the CPU, has no such
  query in any iteration of any case below (0 candidates among 10k - 530k queries per case;
  counted with _near_tie_candidates), so nothing may be excused.  Whoever changes a seed, a
  size or a parameter value recounts first and keeps only inputs with 0 candidates.
* 1e-10 on scaling_factor: the radius is an exact max; only the centroid's summation order
  differs, by at most n * 2^-53 * max|p| ~ 6e-13 for n <= 5000.
* compare_traces' DIST_NOISE = 1e-12 stays valid: with beta <= 4 and scale <= 10 normalized
  coordinates are <= 40 and their f64 noise <= 1e-14.

A traced run walks the loop without look-ahead (engine.cpp: lag 0), so every case also runs
untraced, where the host queues the NN grids one iteration ahead (do_se3 / do_r3), and the
two results must be bitwise equal.
"""
import numpy as np
import pytest

from test_gpu_parity import _se3_vectors, _tie_ok
from test_gpu_trace import DIST_NOISE, NEAR_TIE_REL, compare_traces

pytestmark = pytest.mark.gpu

VARIANTS = ["pt2pt", "pt2pl", "gicp"]
B_BASE = dict(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
              number_of_nn_for_LRF=60)
R_BASE = dict(estimated_overlap=0.75, max_num_se3_iterations=10, mse_switch_error=5e-5, number_of_nn_for_LRF=90)

ALPHAS = [0.0, 0.01, 0.3, 1.0, 7.0, 50.0, 1000.0]
BETA_SCALE = [(0.25, 3.0), (4.0, 3.0), (1.0, 0.5), (1.0, 10.0), (2.0, 1.5)]
CF_ALPHA_BETA = [(3.0, 0.5), (3.0, 2.0), (0.0, 1.0), (0.3, 3.0), (25.0, 1.0)]
ITER_CAPS = [4, 10, 11, 12]
SE3_CAPS = [(1, "gicp"), (3, "pt2pl")]
OVERLAPS = [(0.05, 177), (0.5, 1772), (0.9997, 3542), (1.5, 3544)]
NN_WEIGHTS = [(0.0, 1.0, 1.0), (0.01, 1.0, 1.0), (50.0, 1.0, 1.0), (1000.0, 1.0, 1.0), (3.0, 0.5, 1.0),
              (3.0, 4.0, 1.0)]
BATCH_SEEDS = [2, 3, 4]
BATCH_OVER = dict(alpha_rot=0.05, beta_transl=2.0)
PLUMBING_OVER = dict(alpha_rot=7.0, beta_transl=0.25, scale_preprocessing=1.5)


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
def pair_b(bunny_unique):
    from se3icp import datasets
    src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=2, subsample=0.1)
    assert (src.shape[0], tgt.shape[0]) == (3544, 3563)
    return src, tgt


@pytest.fixture(scope="module")
def pair_r():
    from se3icp import datasets
    src, tgt = datasets.rgbd_pairs(1, seed=5, stride=8)[0][0]
    assert (src.shape[0], tgt.shape[0]) == (4413, 4397)
    return src, tgt


def _near_tie_candidates(ref):
    """Queries of an oracle trace that compare_traces would excuse if the GPU picked the
    runner-up: the oracle's two best targets within a rounding-level gap."""
    n = 0
    for it in range(ref["num_iterations"]):
        d2a, d2b = ref["corr_d2"][it], ref["corr_d2b"][it]
        n += int(((d2b - d2a) <= NEAR_TIE_REL * d2a + DIST_NOISE ** 2).sum())
    return n


def _oracle(refcpu, src, tgt, rkind, rvariant, params):
    return refcpu.register(src, tgt, rkind, rvariant, refcpu.default_params(**params), trace_iters=160,
                           trace_margins=True)


def _traced_case(se3icp_mod, refcpu, parity_record, label, pair, method, rkind, rvariant, params, ref=None):
    """One traced GPU run against the oracle with the assertions every case makes; returns
    (GPU result, GPU trace, oracle run, counters)."""
    src, tgt = pair
    overlap = params.get("estimated_overlap", 1.0)
    if ref is None:
        ref = _oracle(refcpu, src, tgt, rkind, rvariant, params)
    gp = se3icp_mod.default_params(**params)
    res, gtr = se3icp_mod.register_batch_traced([(src, tgt)], method, gp, pair=0, max_iters=160)
    g = res[0]
    dpose = float(np.linalg.norm(g.T - ref["T"]))
    sf_ref = 1.0 if rkind == refcpu.RUN_ICP else ref["scaling_factor"]
    print(f"[params] {label}: iterations gpu {g.num_iterations}/{g.num_pure_se3_iterations} oracle "
          f"{ref['num_iterations']}/{ref['num_pure_se3_iterations']}, |T_gpu - T_ref|_F {dpose:.3e}, "
          f"scaling_factor gpu {g.scaling_factor!r} oracle {sf_ref!r}, rechecked {g.num_rechecked}")
    assert g.status == 0
    assert g.num_iterations == ref["num_iterations"], label
    assert g.num_pure_se3_iterations == ref["num_pure_se3_iterations"], label
    tot = compare_traces(gtr, ref, overlap, label)
    assert tot["idx_diff"] == 0, (label, tot)  # the oracle has no near-tie here: nothing to excuse
    assert dpose <= 1e-5, (label, dpose)
    if rkind == refcpu.RUN_ICP:
        assert g.scaling_factor == 1.0
    else:
        assert abs(g.scaling_factor - sf_ref) <= 1e-10 * sf_ref, (label, g.scaling_factor, sf_ref)
    # the same run with the host's one-iteration look-ahead (no trace armed)
    plain = se3icp_mod.register_batch([(src, tgt)], method, gp)[0]
    assert np.array_equal(plain.T, g.T), (label, "untraced run differs", plain.T, g.T)
    assert (plain.num_iterations, plain.num_pure_se3_iterations, plain.scaling_factor) == \
        (g.num_iterations, g.num_pure_se3_iterations, g.scaling_factor), label
    parity_record("params: " + label, iterations=int(ref["num_iterations"]),
                  pure_se3_iterations=int(ref["num_pure_se3_iterations"]), queries=tot["queries"],
                  idx_diff=tot["idx_diff"], dist_ulp1=tot["dist_ulp1"], kept_swaps=tot["kept_swaps"],
                  max_pose_diff=tot["max_pose_diff"], rechecked_queries=int(g.num_rechecked))
    return g, gtr, ref, tot


# --------------------------------------------------------------------------- 1. weights
@pytest.mark.parametrize("i", range(len(ALPHAS)), ids=[f"alpha{a:g}" for a in ALPHAS])
def test_alpha_rot_sweep(se3icp_mod, refcpu, pair_b, parity_record, i):
    """alpha_rot over the reference's grid: alpha = 0 builds the 12-D tree over nine
    dimensions of zero extent, alpha = 1000 gives f32_err vector norms of ~1732 where the
    default's are ~6, and every value but 3 separates alpha^2 from the default's 9 in
    prep_settle's certificate (an engine built with the constant 9, or with alpha, there
    fails the cases alpha = 7, 50 and 1000)."""
    alpha, variant = ALPHAS[i], VARIANTS[i % 3]
    params = dict(B_BASE, alpha_rot=alpha)
    _, _, ref, _ = _traced_case(se3icp_mod, refcpu, parity_record, f"B se3_{variant} alpha {alpha:g}", pair_b,
                                "se3_" + variant, refcpu.RUN_SE3_ICP, variant, params)
    if alpha == 0.0:
        # rotations carry no weight: the R3 phase never meets the MSE criterion and this is
        # the suite's only GPU run that ends at max_num_iterations_ = 150
        assert ref["num_iterations"] == 150


@pytest.mark.parametrize("i", range(len(BETA_SCALE)), ids=[f"beta{b:g}-scale{s:g}" for b, s in BETA_SCALE])
def test_beta_transl_and_scale_sweep(se3icp_mod, refcpu, pair_b, parity_record, i):
    """beta != 1: the translation rows are no longer the points (k_lrf8, k_lrf and k_knn_big
    each write them); scale != 3: `mse_rel < sf * mse` and the de-normalization use the
    device-computed scale."""
    (beta, scale), variant = BETA_SCALE[i], VARIANTS[i % 3]
    params = dict(B_BASE, beta_transl=beta, scale_preprocessing=scale)
    _traced_case(se3icp_mod, refcpu, parity_record, f"B se3_{variant} beta {beta:g} scale {scale:g}", pair_b,
                 "se3_" + variant, refcpu.RUN_SE3_ICP, variant, params)


def test_se3_pure_at_sweep_weights(se3icp_mod, refcpu, pair_b, parity_record):
    params = dict(B_BASE, alpha_rot=0.5, beta_transl=2.0, scale_preprocessing=1.5)
    _, gtr, _, _ = _traced_case(se3icp_mod, refcpu, parity_record, "B se3_pure_pt2pl alpha 0.5 beta 2 scale 1.5",
                                pair_b, "se3_pure_pt2pl", refcpu.RUN_SE3_PURE, "pt2pl", params)
    assert set(gtr["phase"].tolist()) == {1}


# --------------------------------------------------------------------------- 2. confidence variant
@pytest.mark.parametrize("alpha,beta", CF_ALPHA_BETA)
def test_cf_variant_at_sweep_weights(se3icp_mod, refcpu, pair_r, parity_record, alpha, beta):
    """run_se3_icp_with_cf (ISR.cpp:742-959): source rows beta * t, target search rows the
    unweighted points, stored distance against the target's beta * t.  With beta != 1 the
    three differ from one another; at beta = 1 they coincide."""
    params = dict(R_BASE, alpha_rot=alpha, beta_transl=beta)
    _traced_case(se3icp_mod, refcpu, parity_record, f"R se3_gicp_with_cf alpha {alpha:g} beta {beta:g}", pair_r,
                 "se3_gicp_with_cf", refcpu.RUN_SE3_ICP_CF, "gicp", params)


@pytest.mark.parametrize("case", ["B", "R-cf"])
def test_every_frame_kernel_writes_the_same_weighted_rows(se3icp_mod, refcpu, pair_b, pair_r, case):
    """k_lrf8, k_lrf and k_knn_big each write the alpha/beta-weighted rows with their own copy
    of the code; the default setup uses the first (and hands some points to the second).
    With beta != 1 and alpha != 3 the exact kernel (mode 1) and the global-buffer kernel
    (mode 2) must give bitwise the default's result, which matches the oracle."""
    if case == "B":
        pair, method, rkind, variant = pair_b, "se3_pt2pl", refcpu.RUN_SE3_ICP, "pt2pl"
        params = dict(B_BASE, alpha_rot=0.5, beta_transl=2.0, scale_preprocessing=1.5)
    else:
        pair, method, rkind, variant = pair_r, "se3_gicp_with_cf", refcpu.RUN_SE3_ICP_CF, "gicp"
        params = dict(R_BASE, alpha_rot=0.3, beta_transl=3.0)
    from se3icp import registration
    gp = se3icp_mod.default_params(**params)
    ref = refcpu.register(*pair, rkind, variant, refcpu.default_params(**params))
    runs = []
    try:
        for mode in (0, 1, 2):
            registration.set_lrf_exact(mode)
            runs.append(se3icp_mod.register_batch([pair], method, gp)[0])
    finally:
        registration.set_lrf_exact(0)
    assert np.linalg.norm(runs[0].T - ref["T"]) <= 1e-5
    assert (runs[0].num_iterations, runs[0].num_pure_se3_iterations) == \
        (ref["num_iterations"], ref["num_pure_se3_iterations"])
    for mode, r in enumerate(runs):
        assert np.array_equal(r.T, runs[0].T), (case, mode, r.T, runs[0].T)
        assert (r.num_iterations, r.num_pure_se3_iterations) == \
            (runs[0].num_iterations, runs[0].num_pure_se3_iterations), (case, mode)


# --------------------------------------------------------------------------- 3. iteration caps
@pytest.mark.parametrize("cap", ITER_CAPS)
def test_max_num_iterations_cap(se3icp_mod, refcpu, pair_b, parity_record, cap):
    """The reference tests `num_iterations_ == max_num_iterations_` only in the R3 branch
    (ISR.cpp:726): a pair that switches at iteration 10 never meets a cap of 4 or 10 and runs
    on to the MSE criterion; 11 and 12 bind."""
    params = dict(B_BASE, max_num_iterations=cap)
    ref = _oracle(refcpu, *pair_b, refcpu.RUN_SE3_ICP, "pt2pl", params)
    if cap <= 10:
        assert ref["num_iterations"] > cap, (cap, ref["num_iterations"])  # the cap is passed by
    else:
        assert ref["num_iterations"] == cap, (cap, ref["num_iterations"])  # the cap binds
    _traced_case(se3icp_mod, refcpu, parity_record, f"B se3_pt2pl max_num_iterations {cap}", pair_b, "se3_pt2pl",
                 refcpu.RUN_SE3_ICP, "pt2pl", params, ref=ref)


@pytest.mark.parametrize("cap,variant", SE3_CAPS)
def test_max_num_se3_iterations_cap(se3icp_mod, refcpu, pair_b, parity_record, cap, variant):
    params = dict(B_BASE, max_num_se3_iterations=cap)
    _, gtr, ref, _ = _traced_case(se3icp_mod, refcpu, parity_record,
                                  f"B se3_{variant} max_num_se3_iterations {cap}", pair_b, "se3_" + variant,
                                  refcpu.RUN_SE3_ICP, variant, params)
    assert ref["num_pure_se3_iterations"] == cap
    assert gtr["phase"].tolist() == [1] * cap + [2] * (ref["num_iterations"] - cap)


def test_run_icp_iteration_cap(se3icp_mod, refcpu, pair_b, parity_record):
    params = dict(B_BASE, max_num_iterations=3)
    g, _, ref, _ = _traced_case(se3icp_mod, refcpu, parity_record, "B gicp max_num_iterations 3", pair_b, "gicp",
                                refcpu.RUN_ICP, "gicp", params)
    assert ref["num_iterations"] == 3 and g.num_pure_se3_iterations == -1


# --------------------------------------------------------------------------- 4. overlap edges
@pytest.mark.parametrize("overlap,n_kept", OVERLAPS)
def test_estimated_overlap_edges(se3icp_mod, refcpu, pair_b, parity_record, overlap, n_kept):
    """nkeep near 1 and near n, and a ratio above 1, which PCL clamps to 1 (no trim: the
    recorded cut is UINT64_MAX, which compare_traces asserts for overlap >= 1)."""
    params = dict(B_BASE, estimated_overlap=overlap)
    _, gtr, ref, _ = _traced_case(se3icp_mod, refcpu, parity_record, f"B se3_pt2pt overlap {overlap:g}", pair_b,
                                  "se3_pt2pt", refcpu.RUN_SE3_ICP, "pt2pt", params)
    assert (ref["n_kept"][:ref["num_iterations"]] == n_kept).all()
    if overlap >= 1.0:
        assert (gtr["trim_key"] == np.iinfo(np.uint64).max).all()


# --------------------------------------------------------------------------- 5. all-equal trim keys
@pytest.mark.parametrize("method", ["pt2pt", "se3_pt2pt"])
def test_trim_of_all_equal_keys(se3icp_mod, refcpu, fixture_clouds, parity_record, method):
    """The fixture against a copy of itself: in iteration 1 every float distance is exactly
    0.0, so all 4167 keys (more than kTrimList = 4096) share every distance bit and k_trim's
    radix passes must resolve the cut in the index bits: the key of rank nkeep - 1 is the
    index nkeep - 1.  Iteration 2 opens a window at d_prev = 0 that holds nothing; its
    distances are f64 rounding noise (~4e-15), so the trimmed sets are not compared there."""
    src = fixture_clouds[0]
    tgt = src.copy()
    n = src.shape[0]
    nkeep = int(np.floor(np.float32(0.5) * np.float32(n)))
    assert n > 4096 and nkeep == 2083
    se3 = method.startswith("se3_")
    params = dict(estimated_overlap=0.5, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                  number_of_nn_for_LRF=90)
    ref = _oracle(refcpu, src, tgt, refcpu.RUN_SE3_ICP if se3 else refcpu.RUN_ICP, "pt2pt", params)
    gp = se3icp_mod.default_params(**params)
    res, gtr = se3icp_mod.register_batch_traced([(src, tgt)], method, gp, pair=0, max_iters=160)
    g = res[0]
    dpose = float(np.linalg.norm(g.T - ref["T"]))
    print(f"[params] F self {method}: iterations gpu {g.num_iterations} oracle {ref['num_iterations']}, "
          f"trim_key {gtr['trim_key'][:2]}, |T_gpu - T_ref|_F {dpose:.3e}, iteration-1 index differences "
          f"{int((gtr['corr_idx'][0] != ref['corr_idx'][0]).sum())}, nonzero distances "
          f"{int((gtr['corr_dist'][0] != 0).sum())}")
    assert ref["num_iterations"] == 2
    assert g.num_iterations == ref["num_iterations"]
    assert g.num_pure_se3_iterations == ref["num_pure_se3_iterations"]
    assert len(gtr["phase"]) == 2
    # exact ties inside the duplicate groups go to the lowest index on both sides
    assert np.array_equal(gtr["corr_idx"][0], ref["corr_idx"][0])
    assert (ref["corr_idx"][0] != np.arange(n)).sum() > 0  # the duplicates are there
    assert (gtr["corr_dist"][0] == 0.0).all() and (ref["corr_dist"][0] == 0.0).all()
    assert ref["n_kept"][0] == nkeep
    assert int(gtr["trim_key"][0]) == nkeep - 1
    assert dpose <= 1e-9, dpose
    if se3:
        assert abs(g.scaling_factor - ref["scaling_factor"]) <= 1e-10 * ref["scaling_factor"]
    else:
        assert g.scaling_factor == 1.0
    plain = se3icp_mod.register_batch([(src, tgt)], method, gp)[0]
    assert np.array_equal(plain.T, g.T) and plain.num_iterations == g.num_iterations
    parity_record(f"params: F self {method} overlap 0.5", iterations=int(ref["num_iterations"]), queries=2 * n,
                  idx_diff=int((gtr["corr_idx"][0] != ref["corr_idx"][0]).sum()), trim_key_0=int(gtr["trim_key"][0]),
                  max_pose_diff=dpose, rechecked_queries=int(g.num_rechecked))


# --------------------------------------------------------------------------- 6. stage NN
@pytest.fixture(scope="module")
def fixture_frames(refcpu, fixture_clouds):
    src, tgt = fixture_clouds
    return refcpu.toldi_frames(src, 90), refcpu.toldi_frames(tgt, 90)


@pytest.mark.parametrize("alpha,beta_q,beta_d", NN_WEIGHTS)
def test_se3_nn_at_sweep_weights(se3icp_mod, refcpu, fixture_frames, parity_record, alpha, beta_q, beta_d):
    """The 12-D search entry on weighted fixture frames (the last two cases are the cf
    layout: weighted query translation, unweighted target).  d2 must be bit-equal, as
    test_adversarial_near_ties_at_120k demands of the same entry.

    The bar on the f64 recheck.  A query whose nearest target is one of several identical
    rows can never be certified in f32 (the candidates' f32 distances are the same bits), so
    at least those queries must reach the recheck: 161, 161, 186, 193, 248 and 139 of the
    4167 in the six cases, counted from the oracle's answer.  No larger share follows from
    f32 rounding, not even at alpha = 1000, where one might expect the recheck to carry the
    whole search (u * 1000 ~ 6e-5 absolute per rotation entry against translation gaps of
    ~1e-2): f32 precision is relative, and the frames of neighbouring targets differ, so the
    2-NN gap grows with alpha^2 as the rounding error does.  With f32_err evaluated in f64
    on the oracle's 2-NN margins the median gap is 9e4 times the error at alpha = 1000 (3e3
    at alpha = 0) and `gap <= 2 f32_err` holds for 193 queries, the duplicates and no other.
    The MI355X measured exactly those: 161 / 161 / 186 / 193 rechecked at alpha 0 / 0.01 /
    50 / 1000 (under 5 %, not half).  It follows that these cases cannot tell whether
    f32_err is given the right vector norms at alpha = 1000 (an engine built with the norms
    capped at 12 passes them): that needs near-ties at large norms,
    test_adversarial_near_ties_at_120k's construction at alpha = 1000, which this file does
    not have."""
    fs, ft = fixture_frames
    q = _se3_vectors(fs, alpha, beta_q)
    d = _se3_vectors(ft, alpha, beta_d)
    gi, gd2, nrech = se3icp_mod.nearest_neighbors(q, d)
    ri, rd2 = refcpu.nn(q, d)
    mism = np.nonzero(gi != ri)[0]
    nq = q.shape[0]
    _, inv, cnt = np.unique(d, axis=0, return_inverse=True, return_counts=True)
    must = int((cnt[inv.ravel()[ri]] > 1).sum())
    print(f"[params] F nn alpha {alpha:g} beta {beta_q:g}/{beta_d:g}: {nq} queries, {nrech} rechecked in f64 "
          f"(at least {must} uncertifiable), {mism.size} index differences, {int((gd2 != rd2).sum())} d2 bit "
          f"differences")
    parity_record(f"params: F nn alpha {alpha:g} beta {beta_q:g}/{beta_d:g}", queries=nq, rechecked_f64=int(nrech),
                  uncertifiable_queries=must, index_differences=int(mism.size),
                  d2_bit_differences=int((gd2 != rd2).sum()))
    for i in mism:
        assert _tie_ok(d, q[i], gi[i], ri[i], rd2[i], 12), (i, gi[i], ri[i])
    assert np.array_equal(gd2, rd2)
    assert nrech >= must, (nrech, must)


# --------------------------------------------------------------------------- 7. plumbing and batching
def test_class_attributes_reach_the_engine(se3icp_mod, refcpu, pair_b, parity_record):
    """alpha_rot, beta_transl and scale_preprocessing set as attributes of the reference-shaped
    class give bitwise the register_batch result of the same Params."""
    src, tgt = pair_b
    params = dict(B_BASE, **PLUMBING_OVER)
    g, _, _, _ = _traced_case(se3icp_mod, refcpu, parity_record, "B se3_gicp alpha 7 beta 0.25 scale 1.5", pair_b,
                              "se3_gicp", refcpu.RUN_SE3_ICP, "gicp", params)
    reg = se3icp_mod.IterativeSE3Registration()
    reg.setSourceCloud(src)
    reg.setTargetCloud(tgt)
    reg.estimated_overlap_ = 0.7
    reg.max_num_se3_iterations_ = 10
    reg.mse_ = 1e-5
    reg.mse_switch_error_ = 5e-5
    reg.number_of_nn_for_LRF_ = 60
    reg.alpha_rot = 7.0
    reg.beta_transl = 0.25
    reg.scale_preprocessing = 1.5
    assert (reg.alpha_rot, reg.beta_transl, reg.scale_preprocessing) == (7.0, 0.25, 1.5)
    assert reg.run_se3_icp("gicp") == 0
    assert np.array_equal(reg.current_estimated_T_, g.T)
    assert (reg.num_iterations_, reg.num_pure_se3_iterations_) == (g.num_iterations, g.num_pure_se3_iterations)


def test_batch_at_sweep_weights_equals_single_pairs(se3icp_mod, refcpu, bunny_unique, pair_b, parity_record):
    from se3icp import datasets
    pairs = [datasets.bunny_pair(bunny_unique, seed=s, subsample=0.1)[:2] for s in BATCH_SEEDS]
    assert np.array_equal(pairs[0][0], pair_b[0])
    params = dict(B_BASE, **BATCH_OVER)
    got = se3icp_mod.register_batch(pairs, "se3_gicp", se3icp_mod.default_params(**params))
    for seed, pair, b in zip(BATCH_SEEDS, pairs, got):
        g, _, _, _ = _traced_case(se3icp_mod, refcpu, parity_record, f"B seed {seed} se3_gicp alpha 0.05 beta 2",
                                  pair, "se3_gicp", refcpu.RUN_SE3_ICP, "gicp", params)
        assert np.array_equal(b.T, g.T), (seed, b.T, g.T)
        assert (b.num_iterations, b.num_pure_se3_iterations, b.scaling_factor) == \
            (g.num_iterations, g.num_pure_se3_iterations, g.scaling_factor), seed
