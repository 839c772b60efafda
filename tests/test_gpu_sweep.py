"""GPU tests of the parameter sweep (se3icp_register_sweep): one shared setup, the variants
in groups, every result bitwise what a separate register_batch call returns.

The bar needs no oracle and no tolerance: a pair registers bit for bit the same alone or in
any batch (test_gpu_params.py::test_batch_at_sweep_weights_equals_single_pairs), the sweep's
shared setup stores the unweighted SE(3) rows (alpha = beta = 1: 1.0 * x is exact) and
k_sweep_expand weights them with the arithmetic of the frame kernels' epilogue.  So every
comparison below is numpy.array_equal / == against register_batch on the same build, over T,
num_iterations, num_pure_se3_iterations, status and scaling_factor (num_rechecked and the
times are left out: they are diagnostics of the batch a pair ran in).

Inputs (a few thousand points, odd and unequal sizes, so a replica's column segments start
and end inside 16-byte chunks):
  B     datasets.bunny_pair(bunny_unique, seed=s, subsample=0.1), seeds 2, 3, 4
  R     datasets.rgbd_pairs(1, seed=5, stride=8)[0][0]
  tiny  the first 67 source and 129 target points of B seed 2 (number_of_nn_for_LRF = 30),
        batched with full B pairs
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B_BASE = dict(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
              number_of_nn_for_LRF=60)
R_BASE = dict(estimated_overlap=0.75, max_num_se3_iterations=10, mse_switch_error=5e-5, number_of_nn_for_LRF=90)
SEEDS = [2, 3, 4]


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


@pytest.fixture(scope="module")
def pairs_b(bunny_unique):
    from se3icp import datasets
    pairs = [datasets.bunny_pair(bunny_unique, seed=s, subsample=0.1)[:2] for s in SEEDS]
    assert (pairs[0][0].shape[0], pairs[0][1].shape[0]) == (3544, 3563)
    return pairs


@pytest.fixture(scope="module")
def pair_r():
    from se3icp import datasets
    src, tgt = datasets.rgbd_pairs(1, seed=5, stride=8)[0][0]
    assert (src.shape[0], tgt.shape[0]) == (4413, 4397)
    return src, tgt


@pytest.fixture(scope="module")
def pairs_ragged(pairs_b):
    """Two full B pairs around the tiny one: every later cloud starts at an odd slot."""
    tiny = (pairs_b[0][0][:67].copy(), pairs_b[0][1][:129].copy())
    return [pairs_b[0], tiny, pairs_b[1]]


def _key(r):
    return (r.T.tobytes(), r.num_iterations, r.num_pure_se3_iterations, r.status, r.scaling_factor)


def _same(a, b):
    return (np.array_equal(a.T, b.T) and a.num_iterations == b.num_iterations
            and a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.status == b.status
            and a.scaling_factor == b.scaling_factor)


def _separate(mod, pairs, method, variants):
    return [mod.register_batch(pairs, method, v) for v in variants]


def _check(mod, parity_record, name, pairs, method, variants, max_group=0, device=0, separate=None):
    """The sweep against the separate calls; returns (sweep results, separate results)."""
    want = separate if separate is not None else _separate(mod, pairs, method, variants)
    got = mod.register_sweep(pairs, method, variants, device=device, max_group=max_group)
    assert len(got) == len(variants) and all(len(g) == len(pairs) for g in got)
    bad = [(v, p) for v in range(len(variants)) for p in range(len(pairs)) if not _same(got[v][p], want[v][p])]
    g = max_group if max_group else len(variants)
    iters = sorted({r.num_iterations for row in want for r in row})
    print(f"[sweep] {name}: {len(variants)} variants x {len(pairs)} pairs, max_group {max_group}, "
          f"{len(bad)} differ; iterations {iters[0]}..{iters[-1]}")
    parity_record(f"sweep: {name}", variants=len(variants), pairs=len(pairs), max_group=max_group,
                  groups=-(-len(variants) // g), compared=len(variants) * len(pairs), differ=len(bad),
                  distinct_results=len({_key(r) for row in want for r in row}))
    assert not bad, [(v, p, got[v][p], want[v][p]) for v, p in bad[:2]]
    assert all(r.status == 0 for row in got for r in row)
    return got, want


def test_alpha_sweep(se3icp_mod, pairs_b, parity_record):
    """alpha_rot from the ends and the middle of the reference's grid."""
    variants = se3icp_mod.sweep_params(se3icp_mod.default_params(**B_BASE), alpha_rot=[0.0, 0.01, 3.0, 1000.0])
    _, want = _check(se3icp_mod, parity_record, "B se3_gicp alpha", pairs_b, "se3_gicp", variants)
    # the variants are different problems: a sweep that ignored the weights would not pass
    assert len({_key(row[0]) for row in want}) == 4


def test_everything_that_may_vary(se3icp_mod, pairs_b, parity_record):
    base = dict(B_BASE, alpha_rot=3.0)
    over = [dict(beta_transl=0.25), dict(beta_transl=4.0), dict(estimated_overlap=1.0),
            dict(estimated_overlap=0.05), dict(max_num_se3_iterations=1), dict(max_num_iterations=11),
            dict(max_num_iterations=150, mse=1e-7, mse_switch_error=5e-4), dict()]
    variants = [se3icp_mod.default_params(**dict(base, **o)) for o in over]
    assert variants[-1].estimated_overlap == 0.7 and variants[-1].max_num_se3_iterations == 10
    _, want = _check(se3icp_mod, parity_record, "B se3_gicp all fields", pairs_b, "se3_gicp", variants)
    # max_num_iterations = 11 binds: a pair stopped by it runs longer under the last variant
    assert any(a.num_iterations == 11 and b.num_iterations > 11 for a, b in zip(want[5], want[7]))


def test_groups(se3icp_mod, pairs_ragged, parity_record):
    """Five variants as 5 groups of one, as 2 + 2 + 1 and at the engine's choice, over the
    batch with the tiny pair."""
    base = se3icp_mod.default_params(**dict(B_BASE, number_of_nn_for_LRF=30))
    variants = se3icp_mod.sweep_params(base, alpha_rot=[0.3, 1.0, 3.0, 7.0, 50.0],
                                       beta_transl=[1.0, 2.0, 1.0, 0.5, 1.0])
    want = _separate(se3icp_mod, pairs_ragged, "se3_gicp", variants)
    for mg in (1, 2, 0):
        _check(se3icp_mod, parity_record, f"ragged se3_gicp max_group {mg}", pairs_ragged, "se3_gicp", variants,
               max_group=mg, separate=want)


@pytest.mark.parametrize("method", ["se3_pt2pt", "se3_pt2pl", "se3_pure_gicp"])
def test_se3_families(se3icp_mod, pairs_b, parity_record, method):
    variants = se3icp_mod.sweep_params(se3icp_mod.default_params(**B_BASE), alpha_rot=[0.3, 7.0, 3.0],
                                       beta_transl=[1.0, 1.0, 2.0])
    _check(se3icp_mod, parity_record, f"B {method}", pairs_b[:2], method, variants, max_group=2)


def test_cf_targets(se3icp_mod, pair_r, pairs_b, parity_record):
    """run_se3_icp_with_cf: the targets' f32 rows take their translation from the raw point,
    which shows only with beta != 1."""
    variants = se3icp_mod.sweep_params(se3icp_mod.default_params(**R_BASE), beta_transl=[0.5, 2.0, 1.0],
                                       alpha_rot=[3.0, 3.0, 0.3])
    _check(se3icp_mod, parity_record, "R se3_gicp_with_cf", [pair_r], "se3_gicp_with_cf", variants)


def test_vanilla_gicp(se3icp_mod, pairs_b, parity_record):
    """No frames: the sweep shares ingest, trees and normals and varies the loop only."""
    base = se3icp_mod.default_params(**B_BASE)
    variants = se3icp_mod.sweep_params(base, estimated_overlap=[0.7, 1.0, 0.5], mse=[1e-5, 1e-5, 1e-7])
    _, want = _check(se3icp_mod, parity_record, "B gicp", pairs_b[:2], "gicp", variants)
    assert all(r.scaling_factor == 1.0 and r.num_pure_se3_iterations == -1 for row in want for r in row)


def test_trace_in_second_group(se3icp_mod, pairs_ragged, parity_record):
    """Every weighted row to the bit: a wrong frame entry changes float distances long before
    it changes a pose.  Variant 3 of groups (0, 1) (2, 3) (4): the second group's replica."""
    base = se3icp_mod.default_params(**dict(B_BASE, number_of_nn_for_LRF=30))
    variants = se3icp_mod.sweep_params(base, alpha_rot=[0.3, 1.0, 3.0, 7.0, 50.0],
                                       beta_transl=[1.0, 2.0, 1.0, 0.5, 1.0])
    v, p = 3, 2
    res, tr = se3icp_mod.register_sweep_traced(pairs_ragged, "se3_gicp", variants, variant=v, pair=p, max_group=2)
    ref_res, ref_tr = se3icp_mod.register_batch_traced(pairs_ragged, "se3_gicp", variants[v], pair=p)
    assert ref_tr["phase"].shape[0] > 2
    for k in ("corr_idx", "corr_dist", "trim_key", "T", "mse", "phase"):
        assert tr[k].shape == ref_tr[k].shape, k
        assert np.array_equal(tr[k], ref_tr[k]), k
    for q in range(len(pairs_ragged)):
        assert _same(res[v][q], ref_res[q])
    parity_record("sweep: trace variant 3 pair 2 of groups of 2", iterations=int(tr["phase"].shape[0]),
                  correspondences=int(tr["corr_idx"].size))
    # the trace disarmed itself: the next sweep records nothing and runs as usual
    again = se3icp_mod.register_sweep(pairs_ragged, "se3_gicp", variants[3:4])
    assert _same(again[0][p], ref_res[p])


def test_setup_is_shared(se3icp_mod, pairs_b, parity_record):
    variants = se3icp_mod.sweep_params(se3icp_mod.default_params(**B_BASE), alpha_rot=[0.3, 1.0, 3.0, 7.0])
    se3icp_mod.register_batch(pairs_b, "se3_gicp", variants[0])
    one = se3icp_mod.last_kernel_times()
    se3icp_mod.register_sweep(pairs_b, "se3_gicp", variants, max_group=2)
    kt = se3icp_mod.last_kernel_times()
    npts = sum(s.shape[0] + t.shape[0] for s, t in pairs_b)
    assert one["lrf_queries"] == npts
    assert kt["lrf_queries"] == one["lrf_queries"]
    # the loop entries are summed over the groups: four variants search more than one
    assert kt["se3_queries"] > one["se3_queries"]
    parity_record("sweep: shared setup", lrf_queries_sweep=kt["lrf_queries"], lrf_queries_batch=one["lrf_queries"])


def test_device_entry(se3icp_mod, pairs_b, parity_record):
    import torch
    pairs = pairs_b[:2]
    variants = se3icp_mod.sweep_params(se3icp_mod.default_params(**B_BASE), alpha_rot=[0.3, 3.0, 50.0])
    want = se3icp_mod.register_sweep(pairs, "se3_gicp", variants)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_src = torch.from_numpy(np.concatenate([s for s, _ in pairs])).to("cuda", non_blocking=False)
        d_tgt = torch.from_numpy(np.concatenate([t for _, t in pairs])).to("cuda", non_blocking=False)
    so = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    to = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
    got = se3icp_mod.register_sweep_device(d_src.data_ptr(), so, d_tgt.data_ptr(), to, "se3_gicp", variants,
                                           stream=st.cuda_stream)
    st.synchronize()
    assert all(_same(got[v][p], want[v][p]) for v in range(3) for p in range(2))
    parity_record("sweep: device entry", compared=6)


def test_engine_slot(se3icp_mod, pairs_b, parity_record):
    """A further engine of the same GPU (device | slot << 8), whose first call is a sweep."""
    pairs = pairs_b[:2]
    variants = se3icp_mod.sweep_params(se3icp_mod.default_params(**B_BASE), alpha_rot=[0.3, 3.0, 50.0])
    want = se3icp_mod.register_sweep(pairs, "se3_gicp", variants)
    got = se3icp_mod.register_sweep(pairs, "se3_gicp", variants, device=0 | 7 << 8)
    assert all(_same(got[v][p], want[v][p]) for v in range(3) for p in range(2))
    parity_record("sweep: engine slot 7", compared=6)
