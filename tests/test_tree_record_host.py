"""CPU tests of the tree-record checker (tests/tree_cases.py): the numpy model of the build passes
it on every designed input, and every planted defect is reported by the check named for it --
the checker the GPU tests rely on can fail.  Also the exact evaluation of the kernel's box
function against rationals, and where the fused and the two-rounding form differ."""
import numpy as np
import pytest

import tree_cases as T

f32 = np.float32


def _inputs(kind, n, D, scale=1.0):
    g = T.designed(kind, n, D)
    if scale != 1.0:
        g = np.ascontiguousarray(g * scale)
    return T.inputs_3d(g, np.zeros(3)) if D == 3 else T.inputs_12d(g)


def _names(violations):
    return sorted({v.split()[0] for v in violations})


@pytest.fixture(scope="module")
def generic():
    """(inputs, model) at n = 4097 (L = 7, uneven leaves of 32 / 33 points), 3-D and 12-D."""
    out = {}
    for D in (3, 12):
        inp = _inputs("outward", 4097, D)
        out[D] = (inp, T.model_tree(inp))
    return out


# ------------------------------------------------------------------ the box function
def test_fused_inflation_is_the_exact_one():
    rng = np.random.default_rng(1)
    v = np.concatenate([T.tiny_values(), T.box_differing_values(), rng.normal(size=500).astype(f32),
                        (10.0 ** rng.uniform(-24, 4, 1500)).astype(f32), (2.0 ** np.arange(-70, 20)).astype(f32),
                        np.array([0.0, 1.5, -3.0], f32)])
    assert np.array_equal(T.inflation_fused(v).view(np.uint32), T.inflation_exact(v).view(np.uint32))
    lo, hi = T.box_fused(np.zeros(1, f32), np.zeros(1, f32))
    assert lo[0] == -f32(1e-30) and hi[0] == f32(1e-30)


def test_where_the_two_forms_differ():
    """No f32 value of magnitude >= 2^-31 has differing inflations (all 2^23 significands of one
    binade); below that many do, and a few values near 2e-24 have differing boxes."""
    assert T.differing_in_unit_binade().size == 0
    tiny = T.tiny_values()
    assert tiny.size > 50 and tiny.max() < 2.0 ** -31 and tiny.min() >= f32(1e-24)
    w = T.box_differing_values()
    assert w.size >= 1 and f32(1.8198850e-24) in w
    fl, fh = T.box_fused(w, w)
    tl, th = T.box_two_roundings(w, w)
    assert (fl != tl).all()
    # on the tiny values the inflations differ and the boxes do not
    assert T.fused_differs(tiny).all()
    assert np.array_equal(T.box_fused(tiny, tiny)[0], T.box_two_roundings(tiny, tiny)[0])


# ------------------------------------------------------------------ the model passes
@pytest.mark.parametrize("D", [3, 12])
@pytest.mark.parametrize("n", [200, 4097])
@pytest.mark.parametrize("kind", T.KINDS)
def test_model_passes(kind, n, D):
    inp = _inputs(kind, n, D)
    st = {}
    assert T.check_tree(T.model_tree(inp), inp, st) == []
    assert st["c6_strict"] == 0 and st["slack_min_u"] >= 3.0
    if kind == "tworound":
        assert st["fused_differs"] > 0
    if kind == "zero":
        m = T.model_tree(inp)
        assert (m["lo"][:, 2] == -f32(1e-30)).all() and (m["hi"][:, 2] == f32(1e-30)).all()


def test_model_of_a_sparse_and_an_order_only_tree():
    """40 points in the depth-7 tree of a 4097-point neighbour: most leaves and many inner nodes are
    empty; an order-only tree has its order and f64 vectors alone."""
    inp = T.inputs_3d(T.designed("negative", 40, 3), np.zeros(3), n_max=4097)
    st = {}
    assert T.check_tree(T.model_tree(inp), inp, st) == [] and st["empty_leaves"] == 88
    inp = T.inputs_12d(T.designed("binade", 4097, 12))
    m = T.model_tree(inp, order_only=True)
    assert m["lo"] is None and m["pos"] is None and m["written"] == T.expected_written(12, 0, 7)
    assert T.check_tree(m, inp) == []


def test_undefined_frame_of_a_one_point_cloud():
    """A one-point cloud has no frame: its nine rotation entries are NaN, and their box is the
    empty one (the wave's fminf over idle lanes holding +inf skips the NaN)."""
    rows = np.array([[np.nan] * 9 + [0.25, -0.5, 0.0]])
    inp = T.inputs_12d(rows, n_max=64)
    m = T.model_tree(inp)
    assert m["L"] == 0 and np.all(m["lo"][0, :9] == np.inf) and T.check_tree(m, inp) == []
    lo = m["lo"].copy()
    lo[0, 3] = 0.0
    assert _names(T.check_tree(_edit(m, lo=lo), inp)) == ["C3"]


def test_shifted_3d_inputs():
    """A raw-frame cloud: the f32 vectors are float32(xyz - f32_center), the boxes bound the exact
    differences."""
    rng = np.random.default_rng(5)
    off = np.array([4.5e5, 5.4e6, 300.0])
    xyz = rng.normal(size=(600, 3)) * np.array([30.0, 25.0, 3.0]) + off
    inp = T.inputs_3d(xyz, xyz.mean(0))
    assert T.check_tree(T.model_tree(inp), inp) == []
    wrong = T.inputs_3d(xyz, xyz.mean(0) + np.array([0.0, 2.0 ** -10, 0.0]))
    assert "C2" in _names(T.check_tree(T.model_tree(inp), wrong))


# ------------------------------------------------------------------ planted defects
def _edit(t, **kw):
    t = dict(t)
    for k, v in kw.items():
        t[k] = v
    return t


@pytest.mark.parametrize("D", [3, 12])
def test_defect_duplicated_perm_entry(generic, D):
    inp, m = generic[D]
    perm = m["perm"].copy()
    perm[100] = perm[101]
    assert _names(T.check_tree(_edit(m, perm=perm), inp)) == ["C1"]


@pytest.mark.parametrize("D", [3, 12])
def test_defect_pos_off_by_one(generic, D):
    inp, m = generic[D]
    assert _names(T.check_tree(_edit(m, pos=np.roll(m["pos"], 1)), inp)) == ["C1"]
    pos = m["pos"].copy()
    pos[m["perm"][7]] += 1
    v = T.check_tree(_edit(m, pos=pos), inp)
    assert len(v) == 1 and v[0].startswith("C1 pos")


@pytest.mark.parametrize("D", [3, 12])
def test_defect_tvec_row_of_the_neighbouring_point(generic, D):
    inp, m = generic[D]
    tv = m["tvec"].copy()
    x = 1234
    tv[x] = m["vec"][(m["perm"][x] + 1) % m["n"]]
    v = T.check_tree(_edit(m, tvec=tv), inp)
    assert len(v) == 1 and v[0].startswith("C2 tvec")
    t64 = m["tvec64"].copy()
    t64[x, 0] = np.nextafter(t64[x, 0], np.inf)
    v = T.check_tree(_edit(m, tvec64=t64), inp)
    assert len(v) == 1 and v[0].startswith("C2 tvec64")


def _no_inflation(vmin, vmax):
    return np.asarray(vmin, f32), np.asarray(vmax, f32)


def _hi_by_lo(vmin, vmax):
    vmin, vmax = np.asarray(vmin, f32), np.asarray(vmax, f32)
    return vmin - T.inflation_fused(vmin), vmax + T.inflation_fused(vmin)


def _subtract_both(vmin, vmax):
    vmin, vmax = np.asarray(vmin, f32), np.asarray(vmax, f32)
    return vmin - T.inflation_fused(vmin), vmax - T.inflation_fused(vmax)


def _signed(vmin, vmax):
    """lo (1 - c), hi (1 + c): the wrong direction for negative coordinates."""
    vmin, vmax = np.asarray(vmin, f32), np.asarray(vmax, f32)
    return vmin - (vmin * T.C32 + T.A32), vmax + (vmax * T.C32 + T.A32)


@pytest.mark.parametrize("D", [3, 12])
def test_defect_boxes_without_inflation(D):
    """On the inputs 0.49 ulp outside their f32 values the bare f32 extremes do not contain the
    exact values: C5 says so by itself (C3 sees the other bits too)."""
    for n in (200, 4097):
        inp = _inputs("outward", n, D)
        v = T.check_tree(T.model_tree(inp, box=_no_inflation), inp)
        assert any(x.startswith("C5 containment") for x in v) and any(x.startswith("C5 slack") for x in v), v
        assert "C3" in _names(v)


@pytest.mark.parametrize("D", [3, 12])
def test_defect_hi_inflated_by_lo(D):
    for kind in ("outward", "negative", "tiny"):
        inp = _inputs(kind, 4097, D)
        assert "C3" in _names(T.check_tree(T.model_tree(inp, box=_hi_by_lo), inp)), kind
    # where |lo| is far below |hi| the wrong inflation is also too small: C5
    inp = _inputs("tiny", 4097, D)
    assert "C5" in _names(T.check_tree(T.model_tree(inp, box=_hi_by_lo), inp))


@pytest.mark.parametrize("D", [3, 12])
def test_defect_inflation_of_the_wrong_sign(D):
    for box in (_subtract_both, _signed):
        inp = _inputs("negative", 4097, D)
        v = T.check_tree(T.model_tree(inp, box=box), inp)
        assert any(x.startswith("C5 containment") for x in v) and "C3" in _names(v), (box.__name__, v)


@pytest.mark.parametrize("D", [3, 12])
def test_defect_two_rounding_form(D):
    """The uncontracted formula: bitwise another box on the designed values, and only there."""
    inp = _inputs("tworound", 200, D)
    v = T.check_tree(T.model_tree(inp, box=T.box_two_roundings), inp)
    assert _names(v) == ["C3"], v
    for kind in ("outward", "binade", "tiny"):
        inp = _inputs(kind, 4097, D)
        assert T.check_tree(T.model_tree(inp, box=T.box_two_roundings), inp) == []


@pytest.mark.parametrize("D", [3, 12])
def test_defect_inner_node_copies_its_left_child(generic, D):
    inp, m = generic[D]
    lo, hi = m["lo"].copy(), m["hi"].copy()
    h = T.tree_heap(4, 5)
    lo[h], hi[h] = lo[2 * h + 1], hi[2 * h + 1]
    g = h
    while g > 0:  # (the levels above fold what they are given)
        g = (g - 1) // 2
        lo[g], hi[g] = np.minimum(lo[2 * g + 1], lo[2 * g + 2]), np.maximum(hi[2 * g + 1], hi[2 * g + 2])
    v = T.check_tree(_edit(m, lo=lo, hi=hi), inp)
    assert any(x.startswith("C4 inner box: 1 nodes of level 4") for x in v), v
    # its parent, the union of the copy and its sibling, is consistent: one node is blamed by C4;
    # the points of the right child lie outside the copy: C5
    assert sum(x.startswith("C4") for x in v) == 1 and "C5" in _names(v) and "C3" not in _names(v)


@pytest.mark.parametrize("D", [3, 12])
def test_defect_adopter_with_its_donors_boxes(D):
    """The adopter holds the donor's points under a scale 1.3 times the donor's: the donor's order
    is a valid one, the donor's boxes are not its boxes."""
    don = _inputs("outward", 4097, D)
    ado = _inputs("outward", 4097, D, scale=1.3)
    d = T.model_tree(don)
    good = T.finish_model(_edit(d, role=0), ado)
    assert T.check_adopter(good, d) == [] and T.check_tree(good, ado) == [] and T.boxes_differ(good, d)
    bad = _edit(good, lo=d["lo"], hi=d["hi"])
    v = T.check_tree(bad, ado)
    assert "C3" in _names(v) and "C5" in _names(v) and not T.boxes_differ(bad, d)
    stale = _edit(good, tvec=d["tvec"])
    assert "C2" in _names(T.check_tree(stale, ado))
    other = T.model_tree(ado)
    other["perm"] = np.roll(other["perm"], 1)
    assert T.check_adopter(_edit(other, role=0), d) == ["C7 perm: not the donor's"]


@pytest.mark.parametrize("D", [3, 12])
def test_defect_leaf_ranges_by_ceiling(D):
    inp = _inputs("outward", 4097, D)
    assert any(T.first_by_ceiling(4097, 7, i) != T.tree_first(4097, 7, i) for i in range(129))
    v = T.check_tree(T.model_tree(inp, first=T.first_by_ceiling), inp)
    assert any(x.startswith("C3 leaf box") for x in v), v
    # at a power of two both roundings agree
    inp = _inputs("outward", 4096, D)
    assert T.check_tree(T.model_tree(inp, first=T.first_by_ceiling), inp) == []


@pytest.mark.parametrize("D", [3, 12])
def test_defect_points_exchanged_across_sibling_leaves(generic, D):
    """The leftmost point of a leaf and the rightmost of its sibling change places and everything
    is recomputed from the new order: a valid tree with exact boxes, and no median split."""
    inp, m = generic[D]
    L, n = m["L"], m["n"]
    a, mid, b = T.tree_first(n, L, 10), T.tree_first(n, L, 11), T.tree_first(n, L, 12)
    tv = m["tvec"]
    d = int(np.argmax(tv[a:b].max(0) - tv[a:b].min(0)))
    x, y = a + int(np.argmin(tv[a:mid, d])), mid + int(np.argmax(tv[mid:b, d]))
    perm = m["perm"].copy()
    perm[x], perm[y] = perm[y], perm[x]
    t = T.finish_model(_edit(m, perm=perm), inp)
    v = T.check_tree(t, inp)
    assert len(v) == 1 and v[0].startswith(f"C6 split: 1 nodes of level {L - 1}"), v


def test_quantised_form_of_c6(generic):
    """The statement asserted for the engine: points that share a key may sit on either side.  An
    exchange of the two points next to the split passes it when they are within the quantum and
    fails the strict form; the far exchange above fails both."""
    inp, m = generic[3]
    L, n = m["L"], m["n"]
    t = _edit(m, G=1, H=1)
    assert T.level_path(t, 0) == "multipass" and T.level_path(t, 1) == "lds_partition"
    assert T.level_path(t, 3) == "lds_partition" and T.level_path(t, 4) == "sort512"
    assert T.level_path(t, 5) == "sort256" and T.level_path(t, 6) == "sort128"
    assert T.check_tree(t, inp, c6="quantised") == []
    a, mid, b = T.tree_first(n, L, 10), T.tree_first(n, L, 11), T.tree_first(n, L, 12)
    perm = m["perm"].copy()
    perm[a], perm[b - 1] = perm[b - 1], perm[a]
    far = T.finish_model(_edit(t, perm=perm), inp)
    assert _names(T.check_tree(far, inp, c6="quantised")) == ["C6"]


def test_restated_tree_functions():
    """tree_first and its kin at the sizes the GPU cases use (tree.hpp's worked figures)."""
    assert [T.tree_depth_for(n) for n in (1, 64, 65, 129, 2048, 4096, 4097, 8193, 16384)] == [0, 0, 1, 2, 5, 6, 7, 8, 8]
    assert [T.tree_global_levels(n, T.tree_depth_for(n)) for n in (64, 4096, 4097, 8193, 16384)] == [0, 0, 1, 2, 2]
    assert T.tree_multipass_levels(2, 2, 3) == 2 and T.tree_multipass_levels(2, 32, 3) == 0
    assert T.tree_multipass_levels(2, 16, 3) == 1 and T.tree_multipass_levels(2, 32, 12) == 1
    assert T.tree_local_sort_per(4096, 3) == 8 and T.tree_local_sort_per(4097, 3) == 0
    assert sum(T.tree_first(4097, 7, i + 1) - T.tree_first(4097, 7, i) for i in range(128)) == 4097
    assert T.expected_written(12, 0, 0) == T.expected_written(12, 1, 0) | T.TVEC64
