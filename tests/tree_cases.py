"""The checker of the tree record (se3icp_set_tree_record), its designed inputs and a numpy model
of the build (test_gpu_tree_record.py on the GPU, test_tree_record_host.py for the checker alone).

check_tree(tree, inputs) takes one tree of a record (se3icp.tree_record: rec["src3"] ...) and the
f64 vectors the build was given, and returns the list of violations, each starting with the name
of its check.  Every check is exact; none has a tolerance.

  C1 order    perm is a permutation of 0 .. n-1; pos[perm[x]] == x where pos is written.
  C2 vectors  vec is bitwise float32(xyz - f32_center) (3-D; the f64 subtraction, then the cast, as
              k_normalize / k_graph_normalize / Engine::nn_setup do) or float32(rows) (12-D);
              tvec[x] is bitwise vec[perm[x]]; tvec64 / tpt64 are bitwise the f64 inputs at
              perm[x] (12-D: entries 9 .. 11 of the rows), the w of tpt64 is +0.
  C3 leaves   leaf i of level L holds the positions [tree_first(n, L, i), tree_first(n, L, i + 1));
              its box is bitwise box_fused of the minimum and maximum of its f32 vectors per
              coordinate; an empty leaf is [+inf, -inf], and so is a coordinate that is NaN for
              every point of a leaf that is not full (the undefined frame of a one-point cloud:
              fminf over the wave's idle lanes, which hold +inf, skips the NaN).
  C4 inner    lo / hi of heap node h are fminf / fmaxf of its children 2h + 1, 2h + 2, bitwise.
  C5 sound    independent of C3 (below).
  C6 quality  every inner node with two non-empty children has a coordinate d with
              max_left[d] <= min_right[d] over the f32 vectors ("strict"), or, for the engine
              (c6="quantised"), within the quantum of the key its path sorts by (below).
  C7 adopter  check_adopter: the adopter's perm is bitwise its donor's; its own tvec and boxes
              pass C2 - C5 on its own vectors through check_tree.

The kernel's box function.  k_tree_leafbox and k_tree_local write
    lo = lo - (fabsf(lo) * 4.8e-7f + 1e-30f),  hi = hi + (fabsf(hi) * 4.8e-7f + 1e-30f)
and the compiler contracts the inner expression to one v_fma_f32 (this project builds with the
default -ffp-contract=fast for device code): infl = fl32(|v| c + a) with ONE rounding, c =
float32(4.8e-7), a = float32(1e-30), then the f32 subtraction.  inflation_fused evaluates that
exactly: |v| c is a 48-bit product, exact in f64; p + a is taken in f64 with the error term e of
TwoSum, and s + e rounds to f32 as s does unless s is exactly an f32 midpoint, where the sign of
e decides (inflation_exact is the same through rationals).  inflation_two_roundings is the form
the certificate models used to restate (the product rounded, then the sum).  The two differ
only for |v| < 2^-31 (differing_in_unit_binade: no f32 value of [1, 2) has a product with c that
is a rounding midpoint ties-to-even sends down; tiny_values finds values that do differ).

C5, the slack bar (u = 2^-24, half an f32 ulp relative).  What the consumers assume (DESIGN
section 23, note 1 of the search certificate; box_lb of tests/cert_host.cpp and header_model of
tests/certificate_cases.py): a target skipped behind a box had an f32 bound lb >= thr, lb the
sum over the coordinates of max(lo - qf, qf - hi, 0)^2 of the f32 query qf, and from that the
EXACT distance of the f64 query q to every f64 target t below the node is >= the certified
radius.  Per coordinate with qf < lo (the other side mirrors) this needs t - q >= lo - qf up to
what the factor (1 - 2e-6) of the box test absorbs.  With q <= qf + h(qf), h(x) <= u |x| the
half ulp of x's own rounding, it is enough that
    t - lo >= h(qf)                       for every EXACT target coordinate t below the node.
  * qf and lo of one sign and |qf| <= 2 |lo|: h(qf) <= 2 u |lo|.
  * otherwise the gap lo - qf is at least |qf| / 2, h(qf) <= u |qf| is a relative 2^-23 of the
    gap and 2^-22 of its square: inside the 2e-6 of the box test; nothing is asked of the box.
So the bar is  t - lo >= 2 u |lo|  and  hi - t >= 2 u |hi|  for every point below every node, in
exact arithmetic on the exact t (xyz64 - f32_center, or the f64 row entry): the half ulp of the
target's own rounding is inside it because t, not float32(t), is compared.  From the f32 extreme
v of a face that is 3 u |v|: one for the target's rounding, two for the query's.  The kernel
gives 4.8e-7 |v| = 8.05 u |v| less the rounding of its own subtraction (at most u |v| more), so
about 6 u |v| remain in the worst case: the constant has room, and no binade edge changes that
(below 2^k the subtraction lands in the finer binade, above it the result's half ulp is still
u |v|).  For |v| < 1e-30 / 4.8e-7 the absolute term dominates; v = 0 gives [-1e-30, 1e-30].
The exact t: s = fl64(x - c) and the TwoSum error e, t = s + e, compared in long double (64-bit
significand): exact whenever c = 0 or x - c is exact in f64 (every case of the tests; a UTM
cloud about its own centre cancels exactly enough), and otherwise off by 2^-64 |x|, ten orders
below the bar.

C6, what the build guarantees.  No path sorts the f32 coordinate itself: each splits a node by a
stable partition (or a sort) of a KEY, a monotone quantisation of one coordinate d,
    key = (uint) clamp((x_d - lo) * scale, 0, K)       (f32 arithmetic, monotone in x_d),
so every left point's key is <= every right point's, and two points on the wrong sides share a
key.  The quantum 1 / scale is, per path (k_tree.hip):
    multi-pass k_part_* and k_tree_level (levels < G)  extent_d of the node's sampled box / (2^22 - 1)
    LDS partition of k_tree_local (sort_per == 0)      16 sd_d of the sub-node's sample / (2^22 - 1)
    wave sorts of 128 / 256 / 512 keys                  extent_d of the sub-node itself / (2^20 - 1)
with sd_d <= extent_d / 2 and the sampled box inside the node's.  Equal floors of two f32
products mean the products differ by less than 1 plus their rounding (2^-24 2^22 each), so the
statement asserted for the engine is: there is a d with
    max_left[d] - min_right[d] <= 2 Q extent_d(node),  Q = 1 / (2^22 - 1), 8 / (2^22 - 1), 1 / (2^20 - 1),
the extent over the node's f32 vectors.  The wave sorts key over the sub-node's exact extent, so
nothing is clamped there and the statement is unconditional.  (On the other paths a median
inside the clamped tails, beyond 8 sd of the sample mean or outside the sampled box, would
escape it; it needs more than half of a node's points out there: nodes of more than 512 points
with 32 or more sample points, and no case has it.  The wave sorts used the sample's mean +- 8 sd
until this record showed 2 - 12 last-level nodes per tree without a split: DESIGN section 24.)
An order that is not a split at all -- a scrambled leaf, points exchanged between siblings --
fails it unless the points are that close.
The numpy model splits on the f32 values themselves and passes the strict form.
"""
import fractions
import functools

import numpy as np

LD = np.longdouble
F = fractions.Fraction
f32 = np.float32
U = 2.0 ** -24
C32 = f32(4.8e-7)
A32 = f32(1e-30)
K_LEAF = 64                  # kLeafMax
K_LOCAL_MAX = 4096           # kLocalMax
K_TREE_WG_MIN = 32           # kTreeWgMin (12-D: twice)
PERM, POS, VEC, TVEC, TVEC64, TPT64, BOXES = 1, 2, 4, 8, 16, 32, 64
BUILT = -1


# ------------------------------------------------------------------ tree.hpp, restated
def tree_first(n, level, i):
    return (int(n) * int(i)) >> level


def tree_heap(level, i):
    return (1 << level) - 1 + i


def tree_max_node(n, level):
    return (int(n) + (1 << level) - 1) >> level


def tree_depth_for(max_n):
    L = 0
    while tree_max_node(max_n, L) > K_LEAF:
        L += 1
    return L


def tree_global_levels(max_n, L):
    G = 0
    while G < L and tree_max_node(max_n, G) > K_LOCAL_MAX:
        G += 1
    if L - 1 - G > 7:
        G = L - 8
    return G


def tree_multipass_levels(G, builders, D):
    """H of build_trees: the first global levels, while the builders' nodes are fewer than kTreeWgMin."""
    H = 0
    while H < G and (builders << H) < (2 * K_TREE_WG_MIN if D == 12 else K_TREE_WG_MIN):
        H += 1
    return H


def tree_local_sort_per(n, level):
    mx = tree_max_node(n, level)
    return 2 if mx <= 128 else (4 if mx <= 256 else (8 if mx <= 512 else 0))


def level_path(tree, level):
    """Which code splits the nodes of `level` (into level + 1) in this tree's build."""
    if level < tree["H"]:
        return "multipass"
    if level < tree["G"]:
        return "k_tree_level"
    per = tree_local_sort_per(tree["n"], level)
    if per == 0 and (1 << (level - tree["G"])) > 4:  # (k_tree_local's guard: more than kLocalPartSubs sub-nodes)
        per = 8
    return {0: "lds_partition", 2: "sort128", 4: "sort256", 8: "sort512"}[per]


QUANTUM = {"multipass": 1.0 / (2 ** 22 - 1), "k_tree_level": 1.0 / (2 ** 22 - 1), "lds_partition": 8.0 / (2 ** 22 - 1),
           "sort128": 1.0 / (2 ** 20 - 1), "sort256": 1.0 / (2 ** 20 - 1), "sort512": 1.0 / (2 ** 20 - 1)}


def expected_written(D, side, L):
    """The arrays the build produces: a loop source's 12-D tree below depth 0 is its order and its
    f64 translation entries (the f32 input rows exist whatever the tree does with them)."""
    if D == 3:
        return PERM | POS | VEC | TVEC | TVEC64 | TPT64 | BOXES
    if side == 0:
        return (PERM | VEC | TVEC64) if L > 0 else (PERM | POS | VEC | TVEC | TVEC64 | BOXES)
    return PERM | POS | VEC | TVEC | BOXES


# ------------------------------------------------------------------ the box function
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _differ(a, b):
    """Elementwise: the bits differ, a NaN on both sides (the undefined frame of a one-point cloud;
    its payload is nobody's contract) counting as equal."""
    return (_bits(a) != _bits(b)) & ~(np.isnan(a) & np.isnan(b))


def _same(a, b):
    return a.shape == b.shape and not _differ(a, b).any()


def round_f32(x):
    """The f32 nearest the rational x, ties to even."""
    g = f32(float(x))
    cand = [np.nextafter(g, f32(-np.inf)), g, np.nextafter(g, f32(np.inf))]
    return min(cand, key=lambda c: (abs(F(float(c)) - x), int(f32(c).view(np.uint32)) & 1))


def inflation_fused(v):
    """fl32(|v| c + a), one rounding (v_fma_f32), of an f32 array."""
    av = np.abs(np.asarray(v, f32)).astype(np.float64)
    p = av * np.float64(C32)                 # 24 x 24 bits: exact
    a = np.float64(A32)
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)            # TwoSum: p + a == s + e exactly, |e| <= ulp64(s) / 2
    r = s.astype(f32)                        # the one rounding of s (ties to even)
    # s + e rounds as s does unless s is exactly an f32 midpoint; there e decides the side
    with np.errstate(over="ignore", invalid="ignore"):
        d = s - r.astype(np.float64)         # exact
        nb = np.nextafter(r, np.where(d > 0, f32(np.inf), f32(-np.inf)).astype(f32))
        tie = (d != 0) & (d == (nb.astype(np.float64) - r.astype(np.float64)) / 2)
    return np.where(tie & (np.sign(e) == np.sign(d)), nb, r).astype(f32)


def inflation_exact(v):
    """The same through rationals, one value at a time (the cross-check of inflation_fused)."""
    return np.array([round_f32(F(abs(float(x))) * F(float(C32)) + F(float(A32))) for x in np.ravel(v)], f32)


def inflation_two_roundings(v):
    """fl32(fl32(|v| c) + a): the uncontracted form."""
    return np.abs(np.asarray(v, f32)) * C32 + A32


def box_fused(vmin, vmax):
    vmin, vmax = np.asarray(vmin, f32), np.asarray(vmax, f32)
    return vmin - inflation_fused(vmin), vmax + inflation_fused(vmax)


def box_two_roundings(vmin, vmax):
    vmin, vmax = np.asarray(vmin, f32), np.asarray(vmax, f32)
    return vmin - inflation_two_roundings(vmin), vmax + inflation_two_roundings(vmax)


def guarded(box, vmin, vmax):
    """`box` where vmin <= vmax, as the kernel's guard: [+inf, -inf] and NaN are left alone."""
    vmin, vmax = np.array(vmin, f32), np.array(vmax, f32)
    ok = vmin <= vmax
    if ok.any():
        vmin[ok], vmax[ok] = box(vmin[ok], vmax[ok])
    return vmin, vmax


def fused_differs(v):
    """Mask of the f32 values whose fused and two-rounding inflations differ."""
    v = np.asarray(v, f32)
    return _bits(inflation_fused(v)) != _bits(inflation_two_roundings(v))


@functools.lru_cache(maxsize=None)
def differing_in_unit_binade():
    """The f32 values of [1, 2) whose fused and two-rounding inflations differ, by trying all 2^23
    significands.  There the 1e-30 is 2e-24 of the product and can only break an exact tie of the
    48-bit product |v| c that ties-to-even sends down; c's significand admits no such v: the
    array is empty.  Scaling v by 2^k scales the product exactly, and 1e-30 stays below the least
    distance of a 48-bit product from a midpoint, 2^(k - 68), for k >= -31: the two forms write
    the same box for EVERY f32 value of magnitude >= 2^-31 (4.7e-10)."""
    out = []
    for a in range(0, 1 << 23, 1 << 20):
        v = ((np.arange(a, a + (1 << 20), dtype=np.int64) + (1 << 23)) * 2.0 ** -23).astype(f32)
        out.append(v[fused_differs(v)])
    return np.concatenate(out)


def tiny_values():
    """f32 magnitudes between 1e-24 and 2^-31 where the 1e-30 takes part in the rounding and the
    two forms differ."""
    v = (10.0 ** np.linspace(-24, np.log10(2.0 ** -31), 1200)).astype(f32)
    return v[fused_differs(v)]


@functools.lru_cache(maxsize=None)
def box_differing_values():
    """f32 values whose BOX differs between the two forms.  A differing inflation (one ulp of an
    inflation near 1e-30) moves v -+ infl across a rounding boundary of v's own grid only for v
    within about 2^24 1e-30 of zero, and there for about one value in 2^20: the binade of 2^-79
    (1.65e-24 .. 3.3e-24), all 2^23 significands tried, holds a few (1.8198850e-24 is one)."""
    out = []
    for a in range(0, 1 << 23, 1 << 21):
        v = ((np.arange(a, a + (1 << 21), dtype=np.int64) + (1 << 23)) * 2.0 ** (-79 - 23)).astype(f32)
        fl, _ = box_fused(v, v)
        tl, _ = box_two_roundings(v, v)
        out.append(v[_bits(fl) != _bits(tl)])
    return np.concatenate(out)


# ------------------------------------------------------------------ inputs
def inputs_3d(xyz, f32_center, n_max=None):
    """xyz: the f64 points the build was given (the setup record's xyz; the query or data of
    se3icp_nn); f32_center: the setup scalar (se3icp_nn: the data's mean as nn_center forms it)."""
    return {"D": 3, "exact": np.ascontiguousarray(xyz, np.float64), "center": np.asarray(f32_center, np.float64),
            "n_max": n_max}


def inputs_12d(rows, n_max=None):
    return {"D": 12, "exact": np.ascontiguousarray(rows, np.float64), "center": None, "n_max": n_max}


def nn_center(data):
    """Engine::nn_setup's centre of a 3-D call: the data's coordinates summed in order, then / nd."""
    c = np.zeros(3)
    for row in np.asarray(data, np.float64):
        c = c + row
    return c / float(len(data))


def f32_vectors(inp):
    x = inp["exact"]
    return (x - inp["center"]).astype(f32) if inp["D"] == 3 else x.astype(f32)


def exact_vectors(inp):
    """The exact values the f32 vectors stand for, in long double (module docstring)."""
    x = inp["exact"]
    if inp["D"] == 12:
        return x.astype(LD)
    c = np.broadcast_to(inp["center"], x.shape)
    s = x - c
    bb = s - x
    e = (x - (s - bb)) + (-c - bb)
    return s.astype(LD) + e.astype(LD)


# ------------------------------------------------------------------ the checker
def _leaf_ranges(n, L):
    i = np.arange((1 << L) + 1, dtype=np.int64)
    return (n * i) >> L


def _fold(leaf_lo, leaf_hi, L):
    """Per heap node the minimum / maximum over its leaves ([+inf, -inf] for an empty node)."""
    D = leaf_lo.shape[1]
    lo = np.empty(((2 << L) - 1, D), leaf_lo.dtype)
    hi = np.empty_like(lo)
    lo[(1 << L) - 1:], hi[(1 << L) - 1:] = leaf_lo, leaf_hi
    for l in range(L - 1, -1, -1):
        h = np.arange((1 << l) - 1, (2 << l) - 1)
        lo[h] = np.fmin(lo[2 * h + 1], lo[2 * h + 2])
        hi[h] = np.fmax(hi[2 * h + 1], hi[2 * h + 2])
    return lo, hi


def _leaf_extremes(tv, n, L):
    D = tv.shape[1]
    first = _leaf_ranges(n, L)
    lo = np.full((1 << L, D), np.inf, tv.dtype)
    hi = np.full((1 << L, D), -np.inf, tv.dtype)
    for i in range(1 << L):
        a, b = first[i], first[i + 1]
        if b > a:
            # (as the wave's fminf / fmaxf butterfly over 64 lanes, the idle ones holding +-inf: a
            # coordinate that is NaN for every point stays NaN only in a full leaf)
            lo[i], hi[i] = np.fmin.reduce(tv[a:b], 0), np.fmax.reduce(tv[a:b], 0)
            if b - a < K_LEAF:
                lo[i], hi[i] = np.fmin(lo[i], np.inf), np.fmax(hi[i], -np.inf)
    return lo, hi


def check_tree(tree, inp, stats=None, c6="strict", box=box_fused):
    """The violations of C1 - C6 in one tree of a record (module docstring).  stats (a dict):
    filled with the figures of profiles/tree_record_parity.json."""
    out = []
    n, D, L = tree["n"], tree["D"], tree["L"]
    x64 = inp["exact"]
    st = stats if stats is not None else {}
    if D != inp["D"] or x64.shape != (n, D):
        return [f"C2 shape: tree n {n} D {D} against inputs {x64.shape}"]
    if tree["nnodes"] != (2 << L) - 1 or tree_max_node(n, L) > K_LEAF:
        out.append(f"C3 depth: L {L} nnodes {tree['nnodes']} for n {n}")
    if inp.get("n_max") and L != tree_depth_for(inp["n_max"]):
        out.append(f"C3 depth: L {L}, tree_depth_for({inp['n_max']}) = {tree_depth_for(inp['n_max'])}")
    perm, pos = tree["perm"], tree["pos"]
    # ---- C1
    if perm is None:
        return out + ["C1 perm: not recorded"]
    if not np.array_equal(np.sort(perm), np.arange(n, dtype=perm.dtype)):
        return out + [f"C1 perm: not a permutation of 0 .. {n - 1}"]
    if pos is not None and not np.array_equal(pos[perm], np.arange(n, dtype=pos.dtype)):
        out.append(f"C1 pos: pos[perm[x]] != x at {int((pos[perm] != np.arange(n)).sum())} positions")
    # ---- C2
    v32 = f32_vectors(inp)
    if tree["vec"] is not None and not _same(tree["vec"], v32):
        out.append(f"C2 vec: {int(_differ(tree['vec'], v32).any(1).sum())} input rows are not float32 of the f64 inputs")
    tv = v32[perm]
    if tree["tvec"] is not None and not _same(tree["tvec"], tv):
        out.append(f"C2 tvec: {int(_differ(tree['tvec'], tv).any(1).sum())} rows are not vec[perm[x]]")
    t64 = np.ascontiguousarray(x64[perm][:, 9:12] if D == 12 else x64[perm])
    if tree["tvec64"] is not None and not _same(tree["tvec64"], t64):
        out.append("C2 tvec64: not the f64 inputs at perm[x]")
    if tree["tpt64"] is not None:
        want = np.concatenate([t64, np.zeros((n, 1))], 1)
        if not _same(tree["tpt64"], want):
            out.append("C2 tpt64: not (x, y, z, +0) of the f64 inputs at perm[x]")
    # ---- the f32 extremes of every node from the order (what C3, C5's units and C6 use)
    vlo, vhi = _leaf_extremes(tv, n, L)
    first = _leaf_ranges(n, L)
    st["empty_leaves"] = int((first[1:] == first[:-1]).sum())
    nlo, nhi = _fold(vlo, vhi, L)
    lo, hi = tree["lo"], tree["hi"]
    if lo is not None and hi is not None:
        leaf0 = (1 << L) - 1
        full = first[1:] > first[:-1]
        # ---- C3
        wlo, whi = guarded(box, vlo[full], vhi[full])
        bad = _differ(lo[leaf0:][full], wlo) | _differ(hi[leaf0:][full], whi)
        if bad.any():
            out.append(f"C3 leaf box: {int(bad.any(1).sum())} leaves are not the fused box of their f32 extremes")
        e = ~full
        if e.any() and not (np.all(lo[leaf0:][e] == np.inf) and np.all(hi[leaf0:][e] == -np.inf)):
            out.append("C3 empty leaf: not [+inf, -inf]")
        # what the two-rounding form would have written
        tlo, thi = guarded(box_two_roundings, vlo[full], vhi[full])
        flo, fhi = guarded(box_fused, vlo[full], vhi[full])
        st["fused_differs"] = int((_bits(tlo) != _bits(flo)).sum() + (_bits(thi) != _bits(fhi)).sum())
        # ---- C4
        for l in range(L - 1, -1, -1):
            h = np.arange((1 << l) - 1, (2 << l) - 1)
            wl, wh = np.fmin(lo[2 * h + 1], lo[2 * h + 2]), np.fmax(hi[2 * h + 1], hi[2 * h + 2])  # (fminf / fmaxf)
            bad = (_differ(lo[h], wl) & ~((lo[h] == 0) & (wl == 0))) | (_differ(hi[h], wh) & ~((hi[h] == 0) & (wh == 0)))
            if bad.any():
                out.append(f"C4 inner box: {int(bad.any(1).sum())} nodes of level {l} are not the union of their children")
        # ---- C5
        xe = exact_vectors(inp)[perm]
        elo, ehi = _leaf_extremes(xe, n, L)
        elo, ehi = _fold(elo, ehi, L)
        live = np.isfinite(nlo)  # (a node without points has nothing to contain)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            s_lo = np.where(live, elo - lo.astype(LD), LD(0))
            s_hi = np.where(live, hi.astype(LD) - ehi, LD(0))
            if (s_lo < 0).any() or (s_hi < 0).any():
                out.append(f"C5 containment: {int(((s_lo < 0) | (s_hi < 0)).sum())} faces lie inside the exact values below them")
            need_lo = 2 * LD(U) * np.abs(lo.astype(LD))
            need_hi = 2 * LD(U) * np.abs(hi.astype(LD))
            short = live & ((s_lo < need_lo) | (s_hi < need_hi))
            if short.any():
                out.append(f"C5 slack: {int(short.sum())} faces leave less than 2 u |face| beyond the exact values")
            # the figures: slack from the exact extreme in units of u |v|, v the f32 extreme (v != 0)
            units = np.concatenate([(s_lo / (LD(U) * np.abs(nlo.astype(LD))))[live & (nlo != 0)],
                                    (s_hi / (LD(U) * np.abs(nhi.astype(LD))))[live & (nhi != 0)]])
        if units.size:
            st["slack_min_u"], st["slack_max_u"] = float(units.min()), float(units.max())
    elif tree["written"] & BOXES:
        out.append("C3 boxes: written but not recorded")
    # ---- C6
    viol = {}
    paths = {}
    for l in range(L):
        h = np.arange((1 << l) - 1, (2 << l) - 1)
        a, b = 2 * h + 1, 2 * h + 2
        both = np.isfinite(nlo[a][:, 0]) & np.isfinite(nlo[b][:, 0])
        path = level_path(tree, l) if "G" in tree else "model"
        paths[path] = paths.get(path, 0) + int(both.sum())
        if not both.any():
            continue
        with np.errstate(invalid="ignore"):
            # max_left - min_right and the node's extent, of f32 values: exact in f64
            gap = nhi[a][both].astype(np.float64) - nlo[b][both].astype(np.float64)
            ext = (nhi[h][both].astype(np.float64) - nlo[h][both].astype(np.float64))
        strict = (nhi[a][both] <= nlo[b][both]).any(1)
        st["c6_strict"] = st.get("c6_strict", 0) + int((~strict).sum())
        if c6 == "strict":
            ok = strict
        else:
            ok = (gap <= 2.0 * QUANTUM[path] * ext).any(1)
        if not ok.all():
            viol[l] = int((~ok).sum())
    st["split_nodes"] = paths
    for l, k in viol.items():
        out.append(f"C6 split: {k} nodes of level {l} ({level_path(tree, l) if 'G' in tree else 'model'}) have no separating coordinate")
    return out


def check_adopter(tree, donor):
    """C7: the adopter's order is bitwise its donor's (its vectors and boxes go through check_tree)."""
    out = []
    if tree["role"] < 0:
        out.append("C7 role: not an adopter")
    if tree["n"] != donor["n"] or tree["perm"] is None or donor["perm"] is None or \
            tree["perm"].tobytes() != donor["perm"].tobytes():
        out.append("C7 perm: not the donor's")
    return out


def boxes_differ(a, b):
    return a["lo"].tobytes() != b["lo"].tobytes() or a["hi"].tobytes() != b["hi"].tobytes()


# ------------------------------------------------------------------ the numpy model
def model_tree(inp, L=None, order_only=False, box=box_fused, first=tree_first):
    """A median split on the widest f32 coordinate (stable: ties keep their order), leaf ranges by
    `first`, leaf boxes by `box`, inner boxes by union: a record check_tree passes."""
    v32 = f32_vectors(inp)
    x64 = inp["exact"]
    n, D = v32.shape
    L = tree_depth_for(inp.get("n_max") or n) if L is None else L
    perm = np.arange(n, dtype=np.int32)
    for l in range(L):
        for i in range(1 << l):
            a, m, b = first(n, l, i), first(n, l + 1, 2 * i + 1), first(n, l, i + 1)
            if b - a < 2:
                continue
            idx = perm[a:b]
            d = int(np.argmax(v32[idx].max(0).astype(np.float64) - v32[idx].min(0).astype(np.float64)))
            perm[a:b] = idx[np.argsort(v32[idx, d], kind="stable")]
    t = {"n": n, "D": D, "L": L, "nnodes": (2 << L) - 1, "role": BUILT, "perm": perm}
    return finish_model(t, inp, order_only, box, first)


def finish_model(t, inp, order_only=False, box=box_fused, first=tree_first):
    """Everything of a model record that follows from its perm."""
    v32, x64 = f32_vectors(inp), inp["exact"]
    n, D, L, perm = t["n"], t["D"], t["L"], t["perm"]
    t = dict(t)
    t["vec"] = v32
    t["tvec64"] = np.ascontiguousarray(x64[perm][:, 9:12] if D == 12 else x64[perm])
    t["tpt64"] = np.concatenate([t["tvec64"], np.zeros((n, 1))], 1) if D == 3 else None
    t["pos"] = t["tvec"] = t["lo"] = t["hi"] = None
    t["written"] = PERM | VEC | TVEC64 | (TPT64 if D == 3 else 0)
    if order_only:
        return t
    pos = np.empty(n, np.int32)
    pos[perm] = np.arange(n, dtype=np.int32)
    tv = v32[perm]
    lo = np.full((1 << L, D), np.inf, f32)
    hi = np.full((1 << L, D), -np.inf, f32)
    for i in range(1 << L):
        a, b = first(n, L, i), first(n, L, i + 1)
        if b > a:
            lo[i], hi[i] = np.fmin.reduce(tv[a:b], 0), np.fmax.reduce(tv[a:b], 0)
            if b - a < K_LEAF:
                lo[i], hi[i] = np.fmin(lo[i], np.inf), np.fmax(hi[i], -np.inf)
            lo[i], hi[i] = guarded(box, lo[i], hi[i])
    lo, hi = _fold(lo, hi, L)
    t.update(pos=pos, tvec=tv, lo=lo, hi=hi, written=t["written"] | POS | TVEC | BOXES)
    return t


def first_by_ceiling(n, level, i):
    """A leaf range by another rounding than tree_first: ceil(n i / 2^level)."""
    return -((-int(n) * int(i)) >> level)


# ------------------------------------------------------------------ designed vectors
def _ulp32(v):
    v = np.asarray(v, f32)
    return (np.nextafter(np.abs(v), f32(np.inf)) - np.abs(v)).astype(np.float64)


def designed(kind, n, D, seed=0):
    """(n, D) f64 vectors of one designed kind (no subnormal f32 among their roundings):
      zero      coordinate 2 is exactly 0 for every point (boxes [-fl(1e-30), +fl(1e-30)]);
      negative  every coordinate of every point is negative;
      binade    values at +-2^k and one f32 step on either side of them, k = -6 .. 6;
      tiny      magnitudes from 1e-24 to 1, both signs, log-uniform (the absolute term);
      tworound  coordinate 0 holds only +- the few values near 2e-24 on which the fused and the
                two-rounding BOX differ (box_differing_values), so every leaf's extremes there are
                such values; coordinate 1 only magnitudes of 1e-24 .. 4.7e-10 on which the two
                inflations differ (tiny_values; no larger f32 value has that:
                differing_in_unit_binade) though the boxes do not;
      outward   generic f32 values moved 0.49 f32 ulp up or down in f64 (a random side per entry,
                so about half of all leaf extremes lie OUTSIDE the f32 value they round to);
      copies    200 copies of one point among generic ones (zero-extent boxes, ties in every split)."""
    rng = np.random.default_rng(9100 + 17 * seed + D + n)
    g = rng.normal(size=(n, D))
    if kind == "zero":
        g[:, 2] = 0.0
    elif kind == "negative":
        g = -np.abs(g) - 0.01
    elif kind == "binade":
        k = rng.integers(-6, 7, size=(n, D))
        base = (2.0 ** k).astype(f32)
        step = rng.integers(-1, 2, size=(n, D))
        v = np.where(step < 0, np.nextafter(base, f32(0)), np.where(step > 0, np.nextafter(base, f32(np.inf)), base))
        g = v.astype(np.float64) * rng.choice([-1.0, 1.0], size=(n, D))
    elif kind == "tiny":
        g = 10.0 ** rng.uniform(-24, 0, size=(n, D)) * rng.choice([-1.0, 1.0], size=(n, D))
    elif kind == "tworound":
        pool = tiny_values().astype(np.float64)
        pick = pool[rng.integers(0, len(pool), size=(n, D))]
        g[:, 1] = (pick * rng.choice([-1.0, 1.0], size=(n, D)))[:, 1]
        w = box_differing_values().astype(np.float64)
        g[:, 0] = w[rng.integers(0, len(w), size=n)] * rng.choice([-1.0, 1.0], size=n)
    elif kind == "outward":
        v = g.astype(f32)
        g = v.astype(np.float64) + 0.49 * _ulp32(v) * rng.choice([-1.0, 1.0], size=(n, D))
        assert np.array_equal(g.astype(f32), v)
    elif kind == "copies":
        at = rng.permutation(n)[:min(200, n // 2)]
        g[at] = g[at[0]]
    else:
        raise ValueError(kind)
    g = np.ascontiguousarray(g)
    assert (np.abs(g.astype(f32)[g != 0]) > 1.2e-38).all()
    g.setflags(write=False)
    return g


KINDS = ("zero", "negative", "binade", "tiny", "tworound", "outward", "copies")


def symmetric(p, seed=0):
    """p and -p in pairs, each pair in a random order: Engine::nn_setup's running sum returns to
    exactly 0 after every pair, so the centre of this data cloud is exactly 0 and
    float32(x - centre) is float32(x).  (Not p, -p, p, -p: the global levels key over the box of
    every 2^k-th point, which would then see one of the two clusters only and clamp the other.)"""
    flip = np.random.default_rng(9300 + seed).integers(0, 2, len(p)).astype(bool)[:, None]
    out = np.empty((2 * len(p), p.shape[1]))
    out[0::2], out[1::2] = np.where(flip, -p, p), np.where(flip, p, -p)
    return np.ascontiguousarray(out)
