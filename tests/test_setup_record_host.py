"""CPU side of the setup-record tests: the bars of setup_record_cases.py hold for the oracle alone
(f64, sequential sums) on the inputs the GPU tests use, the designed clouds keep their neighbour
lists under the pair's normalization.  (The record's layout against its ctypes mirror:
test_boundary.py.)"""
import numpy as np
import pytest

import lrf_reference as L
import setup_record_cases as S


@pytest.mark.parametrize("name", ["edge", "wrap"])
def test_exact_centres_and_the_planted_radius(name):
    """On the grid clouds the sequential f64 centre IS fsum / n (and so is any other order's), the
    planted point is the pair's farthest by a factor of more than two, it is the last point of
    its cloud, and the oracle's f64 scale is within the bar of the long-double one."""
    pairs = S.edge_pairs() if name == "edge" else S.wrap_pairs()
    assert {c.shape[0] for pr in pairs for c in pr} == set(S.EDGE_SIZES if name == "edge" else (2048, 2049, S.WRAP_SIZE))
    for p, (src, tgt) in enumerate(pairs):
        cs, ct = S.center_exact(src), S.center_exact(tgt)
        for cloud, c in ((src, cs), (tgt, ct)):
            assert np.array_equal(S.center_sequential(cloud).view(np.uint64), c.view(np.uint64))
            assert np.array_equal(S.center_sequential(cloud[::-1]).view(np.uint64), c.view(np.uint64))
        s_ld, (side, at, runner_up) = S.scale_ld(src, tgt, cs, ct, 3.0)
        far_cloud = tgt if side else src
        assert at == far_cloud.shape[0] - 1 and np.array_equal(far_cloud[at], S.FAR), (name, p, side, at)
        assert runner_up < 0.5, (name, p, runner_up)
        dev = S.scale_deviation(S.scale_f64(src, tgt, cs, ct, 3.0), s_ld)
        print(f"[setup record host] {name} pair {p}: oracle scale off by {dev:.3f} bars, runner-up {runner_up:.3f}")
        assert dev <= 1.0, (name, p, dev)
        # a radius about the other cloud's centre, over one cloud only or short of the last point misses
        for wrong in (S.scale_f64(src, tgt, ct, cs, 3.0),
                      S.scale_f64(src if side else tgt, src if side else tgt, cs if side else ct, cs if side else ct, 3.0),
                      S.scale_f64(src[:-1], tgt[:-1], cs, ct, 3.0)):
            assert S.scale_deviation(wrong, s_ld) > 1e6


def test_the_oracle_normalizes_the_smallest_edge_pair_to_the_same_scale():
    from oracle import refcpu
    src, tgt = S.edge_pairs()[0]
    prm = refcpu.default_params(max_num_iterations=1, max_num_se3_iterations=1, number_of_nn_for_LRF=10)
    ref = refcpu.register(src, tgt, refcpu.RUN_SE3_ICP, "pt2pt", prm)
    want = S.scale_f64(src, tgt, S.center_exact(src), S.center_exact(tgt), 3.0)
    assert np.float64(ref["scaling_factor"]).tobytes() == np.float64(want).tobytes()


def test_off_origin_centre_bound_holds_for_the_oracle():
    for p, pair in enumerate(S.utm_pairs()):
        cs = []
        for cloud in pair:
            c, cl = S.center_sequential(cloud), S.center_ld(cloud)
            dev = (np.abs(c.astype(S.LD) - cl) / S.center_bound(cloud, c)).astype(np.float64)
            print(f"[setup record host] utm pair {p} n={cloud.shape[0]}: sequential centre off by {dev.max():.4f} bounds")
            assert (dev <= 1.0).all(), (p, dev)
            # the bound is not vacuous: a centre over n - 1 points is outside it
            c1 = S.center_sequential(cloud[:-1])
            assert (np.abs(c1.astype(S.LD) - cl) > S.center_bound(cloud, c1)).any()
            cs.append(c)
        s_ld, _ = S.scale_ld(pair[0], pair[1], cs[0], cs[1], 3.0)
        assert S.scale_deviation(S.scale_f64(pair[0], pair[1], cs[0], cs[1], 3.0), s_ld) <= 1.0


def test_confidence_bar_holds_for_the_oracle():
    from test_gpu_steps import lounge_confidence
    for src, tgt in S.depth_pairs():
        for cloud in (src, tgt):
            z = cloud[:, 2]
            assert z.min() == 0.4 and z.max() == 4.0
            dev = S.conf_deviation(lounge_confidence(z), z)
            print(f"[setup record host] confidences n={len(z)}: f64 off by {dev.max():.3f} bars")
            assert (dev <= 1.0).all(), float(dev.max())
            assert (S.conf_deviation(lounge_confidence(z) * (1 + 2.0 ** -45), z) > 1.0).all()


def test_designed_clouds_keep_their_neighbours_under_the_pair_scale():
    """The brute-force long-double kNN lists (by (d^2, index)) of the designed clouds normalized as
    the pair (surface517, surface4099) is are those of the raw clouds: the scale creates no tie."""
    (ca, cb), s = S.designed_pair_normalization()
    for kind, c in zip(S.FRAME_KINDS, (ca, cb)):
        raw = L.knn_of(kind)
        got = L.knn_ld(S.normalized(L.cloud(kind), c, s), L.K_MAX)
        assert np.array_equal(got, raw), (kind, np.nonzero((got != raw).any(1))[0][:8])
