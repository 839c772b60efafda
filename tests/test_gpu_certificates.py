"""The NN certificates across iterations against a long-double brute force.

se3icp_nn_sequence runs the loop's own k_nn_prep and search over a given pose sequence and returns,
per step and query, the match, the stored distance and the certificate words.  certificate_cases.py
holds the designed inputs ("aligned pairs": the arg-min flips just where a sound certificate must
refuse to settle), the brute force and the checker; test_cert_host.py asserts on the CPU that the
inputs are not vacuous and that the checker fails on planted defects.  Here every step of every case
is held to the four checks with no tolerance: the result (index, and the stored distance bitwise
away from float rounding midpoints), the search certificate (D1, L2, tightness), the settle
inequality in long double with ring age and phase start, and the absence of a certificate after a
recheck.  The counters show that the group search, the one-query-per-wave search, the recheck and
the settle path were all taken.
"""
import numpy as np
import pytest

import certificate_cases as S

pytestmark = pytest.mark.gpu

WORDS = ("idx", "dist", "cert_d1", "cert_l2", "cert_iter", "cert_j")
FRESH_SLOT = 0 | 13 << 8  # an engine slot no other test of the suite touches


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


def run(mod, case, device=0):
    return mod.nearest_neighbors_sequence(case["query"], case["data"], case["poses"], alpha=case["alpha"],
                                          restart_at=case["restart_at"], device=device)


def record(parity_record, name, case, ref, out, fig, ideal=None):
    fg = S.design_figures(case, ref)
    group = int(out["searched"][out["single"] == 0].sum())
    parity_record("nn_certificate/" + name, steps=fig["steps"], queries=fig["queries"], argmin_changes=fg["changes"],
                  settled=fig["settled"], ideal_settled=ideal, searched_group=group, searched_single=fig["single"],
                  rechecked=fig["rechecked"], ulp1_distances=fig["ulp1"], max_d1_over_d_minus_1=fig["max_d1_slack"],
                  min_1_minus_l2_over_other=fig["min_l2_slack"] if np.isfinite(fig["min_l2_slack"]) else None)


def assert_sound(v):
    assert not any(v.values()), {k: x for k, x in v.items() if x}


@pytest.mark.parametrize("name", sorted(S.main_cases()))
def test_aligned_pairs(se3icp_mod, parity_record, name):
    case = S.main_cases()[name]()
    ref = S.reference(case)
    out = run(se3icp_mod, case)
    v, fig = S.check_run(case, ref, out)
    ideal, ideal_steps = S.ideal_settles(case, ref)
    record(parity_record, name, case, ref, out, fig, ideal)
    print(f"[nn certificate] {name}: settled {fig['settled']} (ideal {ideal}) of {fig['steps'] * fig['queries']}, "
          f"searched {fig['searched']} ({fig['single']} one per wave), rechecked {fig['rechecked']}, "
          f"{fig['ulp1']} 1-ulp distances, D1/d - 1 <= {fig['max_d1_slack']:.3e}, 1 - L2/other >= {fig['min_l2_slack']:.3e}")
    assert_sound(v)
    # every path was taken: the group search, the one-query-per-wave search, the recheck, the settle
    n = fig["queries"]
    assert ((out["single"] == 0) & (out["searched"] >= 256)).any()
    assert ((out["searched"] > 0) & (out["searched"] == out["single"])).any()
    assert (out["rechecked"] > 0).any()
    assert out["searched"][0] == n
    for k, want in enumerate(ideal_steps):
        if want >= 50:
            assert fig["settled_per_step"][k] >= 1, (k + 1, want)
    if case["restart_at"]:
        k = case["restart_at"]
        assert out["searched"][k - 1] == n                          # whatever the certificates allowed
        assert fig["settled_per_step"][k - 2] > 0 and fig["settled_per_step"][k] > 0


@pytest.mark.parametrize("name", sorted(S.size_cases()))
def test_sizes(se3icp_mod, parity_record, name):
    case = S.size_cases()[name]()
    ref = S.reference(case)
    out = run(se3icp_mod, case)
    v, fig = S.check_run(case, ref, out)
    record(parity_record, name, case, ref, out, fig)
    assert_sound(v)
    if len(case["data"]) == 1:  # (the ct.n > 1 guard: a lone target is never certified, nor rechecked)
        assert (out["idx"] == 0).all() and (out["cert_iter"] == -1).all() and (out["rechecked"] == 0).all()


@pytest.mark.parametrize("dim", [3, 12])
def test_exact_ties(se3icp_mod, parity_record, dim):
    case = S.tie_case(dim)
    ref = S.reference(case)
    out = run(se3icp_mod, case)
    v, fig = S.check_run(case, ref, out)
    record(parity_record, "tie%d" % dim, case, ref, out, fig)
    assert_sound(v)
    n = len(case["query"])
    for k, r in enumerate(ref):
        assert r["tie"].all()
        assert np.array_equal(out["idx"][k], np.minimum(r["cand"][:, 0], r["cand"][:, 1]))   # the lowest index
    assert (out["cert_iter"] == -1).all()                           # never a certificate
    assert (out["rechecked"] == n).all() and (out["searched"] == n).all()


def test_ring_age(se3icp_mod, parity_record):
    case = S.ring_case()
    ref = S.reference(case)
    out = run(se3icp_mod, case)
    v, fig = S.check_run(case, ref, out)
    record(parity_record, "ring", case, ref, out, fig)
    assert_sound(v)                                                  # (the results of step 258 among them)
    ci = out["cert_iter"]
    held = int((ci[256] == 2).sum())                                 # after step 257
    print(f"[nn certificate] ring: {held} certificates of step 2 held through step 257; step 258 searched {out['searched'][257]}")
    assert held >= 20
    assert not ((ci[255] == 1) & (ci[256] == 1)).any()              # step 1's: refreshed at step 257
    assert not ((ci[257] >= 0) & (ci[257] <= 2)).any()               # step 2's: refreshed at step 258
    assert out["searched"][257] >= held
    assert (ref[257]["best"] != ref[256]["best"]).sum() >= 10


def test_scheduling_independence(se3icp_mod):
    """The same case on engine slot 0, on a fresh slot whose first call this is (no cost history: its
    cost-ordered dispatch differs) and twice in a row on one slot: bitwise the same."""
    case = S.main_cases()["se3_a3"]()
    runs = [run(se3icp_mod, case, device=FRESH_SLOT), run(se3icp_mod, case), run(se3icp_mod, case),
            run(se3icp_mod, case, device=FRESH_SLOT)]
    for other in runs[1:]:
        for k in WORDS + ("searched", "single", "rechecked"):
            assert runs[0][k].tobytes() == other[k].tobytes(), k
