"""GPU test that no neighbour-selection state crosses calls on one engine.

A graph call that seeds and takes (DESIGN sections 17 and 21) plans its selection as a value
(graph.hpp, SelectPlan) that is handed to the selection and kept only for the lifetime of queued
copies.  The calls around it must not see it: a plain device batch and the stage entries return
the same bits before and after it, and the graph call itself returns the same results and
counters when it runs again behind them.

Inputs are small on purpose: a three-cloud chain of 403, 389 and 301 bunny points whose middle
cloud runs under two pair scales (its second class is seeded from and takes the lists of its
first), and a device batch of two pairs in which two slots have the same point count and other
points, so that the batch is hashed, finds nothing to share and selects on the plain path.  No
point count is a multiple of 8: the last wavefront of every cloud is ragged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def se3icp_mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


def _bytes(r):
    return (r.T.tobytes(), r.num_iterations, r.num_pure_se3_iterations, r.status, np.float64(r.scaling_factor).tobytes())


def test_no_selection_state_crosses_calls(se3icp_mod, bunny_unique):
    import torch
    mod = se3icp_mod
    rng = np.random.default_rng(5)
    pts = np.ascontiguousarray(bunny_unique[rng.permutation(bunny_unique.shape[0])[:2400]], dtype=np.float64)
    cut = lambda o, n, f=1.0: np.ascontiguousarray(pts[o:o + n] * f)
    params = mod.default_params(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=10)

    # the graph: cloud 1 is the target of edge 0 under cloud 0's radius and the source of edge 1
    # under its own
    clouds = [cut(0, 403, 1.7), cut(403, 389), cut(792, 301, 0.6)]
    edges = [(1, 0), (2, 1)]
    # the batch: slots 0 and 3 have 350 points each, and different ones
    pairs = [(cut(1100, 350), cut(1450, 333)), (cut(1783, 297), cut(2050, 350))]
    src = np.ascontiguousarray(np.concatenate([s for s, _ in pairs]))
    tgt = np.ascontiguousarray(np.concatenate([t for _, t in pairs]))
    d_src, d_tgt = torch.from_numpy(src).to("cuda"), torch.from_numpy(tgt).to("cuda")
    torch.cuda.synchronize()
    src_off = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
    tgt_off = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])

    def batch():
        res = mod.register_batch_device(d_src.data_ptr(), src_off, d_tgt.data_ptr(), tgt_off, "se3_gicp", params)
        return [_bytes(r) for r in res], mod.last_seed_stats(), mod.last_take_stats()

    def graph():
        res = mod.register_graph(clouds, edges, "se3_gicp", params)
        return ([_bytes(r) for r in res], mod.last_graph_stats(), mod.last_seed_stats(), mod.last_take_stats(),
                mod.last_tree_stats())

    def stages():
        return mod.knn_self(clouds[1], 10).tobytes(), mod.estimate_normals(clouds[1], 30).tobytes()

    b1 = batch()
    g1 = graph()
    b2 = batch()
    s1 = stages()
    g2 = graph()
    s2 = stages()
    print(f"[call sequence] graph: {g1[1:]}; batch: {b1[1:]}")

    # the graph call shared something: one class seeded and taking, and queries that took
    seed, take = g1[2], g1[3]
    assert seed["classes_seeded"] > 0, seed
    assert take["classes_taking"] > 0 and take["queries_taken"] > 0, take
    assert take["queries_taken"] + take["queries_redone"] == clouds[1].shape[0], take
    # the batch neither seeds nor takes, before or after
    none = {"classes_taking": 0, "queries_taken": 0, "queries_redone": 0, "queries_failed": 0}
    assert b1[1]["classes_seeded"] == 0 and b1[2] == none, b1[1:]
    assert b1 == b2
    assert s1 == s2
    assert g1 == g2, (g1[1:], g2[1:])
