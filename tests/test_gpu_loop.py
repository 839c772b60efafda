"""The per-iteration kernels of k_loop.hip, checked directly: the trimmed rejector's cut on
every code path of k_trim_window / k_trim, the pt2pt sums and solve, the reduction's
structural sizes, and registration away from the origin.

Until this file the loop kernels were seen only through test_gpu_trace.compare_traces, at
whatever inputs the end-to-end cases produce: the kept count, and the kept set up to the
slack of "2 * n_moved swaps".  Here:

A1  assert_exact_cut: trim_key[it] is exactly the nkeep-th smallest of the engine's own keys
    (float bits of corr_dist[it][i]) << 32 | i -- an integer equality against numpy.sort,
    no oracle and no tolerance -- at every iteration of every case of this file.
A2  trim_path_model: a host restatement of the decisions of k_trim_window and k_trim (which
    of their paths an iteration takes).  It only labels iterations; correctness is A1.
A3  synthetic pairs whose keys are designed so that every path is taken: the union of the
    labels over TRIM_CASES must be LABELS and both SETTLED outcomes, asserted on the CPU
    from the oracle's traces and on the GPU from the engine's own.
A4  five of those pairs in one batch, traced pair by pair, against the pairs run alone
    (bitwise), and batches of different sizes repeated on one engine (the per-pair scratch
    trim_ctr / trim_hist / trim_cand and the window word are reset by whichever path ran).
A5  run_icp("pt2pt") recomputed from the trace in numpy.longdouble (two-pass, centred), at
    source sizes on the edges of k_reduce (256 queries per block) and k_reduce_final (18
    chains, 8 loads at a time: the unrolled loop first runs at 127 blocks, a second trip at
    271).  The bar is 10 x the oracle's own deviation from the same recompute.
A6  translation equivariance: registering (src + c, tgt + c) must give S(c) T0 S(-c).

The designed pairs.  The target is three mutually orthogonal planar patches of a jittered
unit lattice, far enough apart that every normal is its patch's; source point i is target
point i moved inside its plane by a designed length, registered with run_icp("pt2pl").  The NN
of source i is target i, its distance is the designed length, and its point-to-plane residual
is zero whatever the length: the solve removes the small rigid motion in iteration 1 and then
stays put, so from iteration 2 on the keys are the designed ones.  (Designed lengths in random
3-D directions under pt2pt do not hold still: with a thousand keys within 2 % of the cut, which
of them are kept depends on the pose to first order, and that feedback has a gain above 1.)
Exactly equal keys are made with duplicated source points (equal in every iteration).
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu

U64MAX = int(np.iinfo(np.uint64).max)
# k_loop.hip / common.hpp constants the model restates
K_TRIM_BLOCKS = 32   # common.hpp kTrimBlocks
K_TRIM_LIST = 4096   # common.hpp kTrimList
K_LOC = 2048         # k_trim_window: kLoc
K_RANK_MAX = 768     # k_trim: kRankMax
K_SPARSE = 96        # k_trim: `else if (cnt < 96u) wv *= 1.5f`
PHASE_SE3, PHASE_R3 = 1, 2

LABELS = ["first/compact", "first/global-count", "hit/rank", "hit/rank-sparse", "hit/wide-lds", "miss/rank-outside",
          "miss/over-4096", "miss/block-over-2048"]
SETTLED = ["distance", "index"]


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


# =========================================================================== A1: the exact cut
def trim_keys(dist):
    """The engine's keys (k_loop.hip trim_key_of): float bits << 32 | query index."""
    d = np.ascontiguousarray(dist, dtype=np.float32)
    return (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(d.shape[0], dtype=np.uint64)


def nkeep_of(n, overlap):
    """floor(float32(ratio) * float32(n)), the ratio clamped to [0, 1] in float32 (engine.cpp:
    `ratio = min(1.0f, max(0.0f, (float)estimated_overlap))`, PCL setOverlapRatio(float))."""
    ratio = min(np.float32(1.0), max(np.float32(0.0), np.float32(overlap)))
    return int(np.floor(np.float32(ratio) * np.float32(n)))


def assert_exact_cut(gtr, n_src, overlap):
    """trim_key[it] == numpy.sort(keys)[nkeep - 1] at every recorded iteration; UINT64_MAX
    when nothing is trimmed; 0 when nothing is kept (k_trim: `if (P->nkeep <= 0)`)."""
    nkeep = nkeep_of(n_src, overlap)
    n_it = len(gtr["phase"])
    assert n_it > 0
    for it in range(n_it):
        got = int(gtr["trim_key"][it])
        assert gtr["corr_dist"][it].shape[0] == n_src
        if nkeep >= n_src:
            want = U64MAX
        elif nkeep <= 0:
            want = 0
        else:
            want = int(np.sort(trim_keys(gtr["corr_dist"][it]))[nkeep - 1])
        assert got == want, (f"iteration {it + 1}: cut {got:#018x} (distance bits {got >> 32:#x}, index "
                             f"{got & 0xffffffff}), want {want:#018x} ({want >> 32:#x}, {want & 0xffffffff}); "
                             f"n {n_src} nkeep {nkeep}")
    return nkeep


# =========================================================================== A2: the host model
def trim_path_model(dists, phases, n, nkeep):
    """Which path k_trim_window / k_trim take in each iteration, replayed in float32 from the
    per-iteration float distances `dists` (the keys' upper halves) and `phases`.

    Restates k_loop.hip:
      * trim_window_state (l. 109-112): the window is void when iter == phase_start, i.e. in
        the first iteration of a phase;
      * k_trim_window (l. 131-136): lo = dprev * (1 - w), hi = dprev * (1 + w) in float32,
        compared on the bit patterns; block `sub` counts the indices [sub * per, sub * per +
        per) with per = ((n + 31) / 32 + 63) & ~63;
      * k_trim_window (l. 170-173): a block holding more than kLoc = 2048 in-window keys adds
        kTrimList + 1 to the pair's count;
      * k_trim (l. 219-231): w starts at 0.02; hit = cnt <= 4096 and nb < k <= nb + cnt; then
        cnt > 768 halves w, a miss multiplies it by 4, a hit on fewer than 96 keys by 1.5,
        and w is capped at 0.9;
      * k_trim (l. 242, 247): a hit on more than kRankMax = 768 keys is resolved by digit
        passes inside LDS, a smaller one by ranking;
      * k_trim (l. 292-307, 314): without a hit the first digit (top 12 key bits) comes from
        the histogram; its bin is compacted into LDS when it holds at most 4096 keys, and
        counted over all keys by further 8-bit digits otherwise;
      * k_trim (l. 389-396): the digits stop as soon as one key is left, so the cut is settled
        by the distance bits unless its distance is shared, and in the index bits then;
      * k_trim (l. 261, 400): the window word keeps the cut's distance bits and the new w.

    Returns one dict per iteration: label (one of LABELS, or "no-trim" / "keep-none"),
    settled ("distance" / "index"), radix ("compact" / "global-count": the path below a
    first iteration or a miss, else None), cnt, below, max_block, bin_count, w (used)."""
    out = []
    if nkeep >= n or nkeep <= 0:
        return [dict(label="no-trim" if nkeep >= n else "keep-none", settled=None, radix=None) for _ in dists]
    per = ((n + K_TRIM_BLOCKS - 1) // K_TRIM_BLOCKS + 63) & ~63
    one = np.float32(1.0)
    dprev, w = None, None
    for it, dist in enumerate(dists):
        bits = np.ascontiguousarray(dist, dtype=np.float32).view(np.uint32)
        assert bits.shape[0] == n
        cut = int(np.sort(trim_keys(dist))[nkeep - 1])
        cut_bits = np.uint32(cut >> 32)
        settled = "index" if int((bits == cut_bits).sum()) > 1 else "distance"
        bin_count = int(((bits >> np.uint32(20)) == (cut_bits >> np.uint32(20))).sum())
        radix = "compact" if bin_count <= K_TRIM_LIST else "global-count"
        void = it == 0 or phases[it] != phases[it - 1] or dprev is None
        rec = dict(settled=settled, bin_count=bin_count, radix=None, cnt=None, below=None, max_block=None)
        if void:
            w = np.float32(0.02)
            rec.update(label="first/" + radix, radix=radix, w=float(w))
        else:
            lo = (dprev * (one - w)).astype(np.float32).view(np.uint32)
            hi = (dprev * (one + w)).astype(np.float32).view(np.uint32)
            inside = (bits >= lo) & (bits <= hi)
            nb = int((bits < lo).sum())
            blocks = [int(inside[b * per:(b + 1) * per].sum()) for b in range(K_TRIM_BLOCKS)]
            cnt = sum(c if c <= K_LOC else K_TRIM_LIST + 1 for c in blocks)
            hit = cnt <= K_TRIM_LIST and nb < nkeep <= nb + cnt
            rec.update(cnt=cnt, below=nb, max_block=max(blocks), w=float(w))
            if hit:
                rec["label"] = "hit/wide-lds" if cnt > K_RANK_MAX else ("hit/rank-sparse" if cnt < K_SPARSE else "hit/rank")
            else:
                rec["radix"] = radix
                if max(blocks) > K_LOC:
                    rec["label"] = "miss/block-over-2048"
                elif cnt > K_TRIM_LIST:
                    rec["label"] = "miss/over-4096"
                else:
                    rec["label"] = "miss/rank-outside"
            if cnt > K_RANK_MAX:
                w = np.float32(w * np.float32(0.5))
            elif not hit:
                w = np.float32(w * np.float32(4.0))
            elif cnt < K_SPARSE:
                w = np.float32(w * np.float32(1.5))
            w = min(w, np.float32(0.9))
        dprev = np.array(cut_bits, dtype=np.uint32).view(np.float32)[()]
        out.append(rec)
    return out


def _near_threshold(rec):
    """The model's counts that sit within 10 % of a threshold they are compared with (a 1-ulp
    distance difference between the engine and the oracle could flip the label there)."""
    bad = []

    def chk(name, v, thr):
        if v is not None and abs(v - thr) <= 0.1 * thr:
            bad.append((name, v, thr))
    if rec["label"].startswith(("first/", "miss/")):
        chk("bin_count", rec["bin_count"], K_TRIM_LIST)
    if rec.get("cnt") is not None and rec["max_block"] <= K_LOC:
        chk("cnt", rec["cnt"], K_SPARSE)
        chk("cnt", rec["cnt"], K_RANK_MAX)
        chk("cnt", rec["cnt"], K_TRIM_LIST)
    if rec.get("max_block") is not None:
        chk("max_block", rec["max_block"], K_LOC)
    return bad


def _fmt_labels(recs):
    return ", ".join(f"{i + 1}:{r['label']}" + (f"[{r['cnt']}/{r['max_block']}]" if r.get("cnt") is not None else
                                                   f"[bin {r.get('bin_count')}]") + ("*" if r["settled"] == "index" else "")
                     for i, r in enumerate(recs))


# =========================================================================== cloud builders
def _rigid(rx, ry, rz, t):
    from se3icp import datasets
    return datasets.make_T(datasets.rot_3d(rx, ry, rz), t)


def _apply(T, pts):
    return np.ascontiguousarray(pts @ T[:3, :3].T + T[:3, 3])


def lattice(n, seed, jitter=0.1):
    """n points of a jittered unit lattice (z fastest, so consecutive indices are neighbours),
    centred on the origin: nearest-neighbour spacing >= 1 - 2 * jitter."""
    m = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)[:n]
    rng = np.random.default_rng(seed)
    p = g.astype(np.float64) + rng.uniform(-jitter, jitter, (n, 3))
    return np.ascontiguousarray(p - p.mean(0))


PLANE_GAP = 8.0  # between the patches: beyond the radius of any point's 30 nearest neighbours in its own patch


def corner_planes(n, seed, jitter=0.1):
    """At least n points on three orthogonal m x m patches of a unit lattice jittered inside its
    plane (patch-major, then rows: consecutive indices are neighbours).  Returns the points and,
    per point, the two in-plane axes."""
    m = int(np.ceil(np.sqrt(n / 3.0)))
    rng = np.random.default_rng(seed)
    ab = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    pts, axes = [], []
    for u, v in ((0, 1), (1, 2), (0, 2)):
        p = np.zeros((m * m, 3))
        p[:, u] = ab[:, 0] + PLANE_GAP + rng.uniform(-jitter, jitter, m * m)
        p[:, v] = ab[:, 1] + PLANE_GAP + rng.uniform(-jitter, jitter, m * m)
        pts.append(p)
        axes.append(np.tile([u, v], (m * m, 1)))
    pts = np.concatenate(pts)
    return np.ascontiguousarray(pts - pts.mean(0)), np.concatenate(axes)


def displaced_source(tgt, axes, lens_by_index, seed, motion):
    """Source point i = motion(target point i + lens[i] * a unit vector inside its plane)."""
    n = len(lens_by_index)
    th = np.random.default_rng(seed).uniform(0, 2 * np.pi, n)
    d = np.zeros((n, 3))
    d[np.arange(n), axes[:n, 0]] = np.cos(th)
    d[np.arange(n), axes[:n, 1]] = np.sin(th)
    return _apply(motion, tgt[:n] + np.asarray(lens_by_index)[:, None] * d)


def shell_lengths(n, k, n_shell, half_width, L0, rng, lo=0.25, hi=2.0, gap=0.12):
    """n sorted lengths: n_shell of them within L0 * (1 +- half_width) on the ranks around k,
    the others below L0 * (1 - gap) and above L0 * (1 + gap)."""
    a = k - n_shell // 2
    b = a + n_shell
    assert 0 < a and b < n
    return np.concatenate([np.sort(rng.uniform(lo * L0, (1 - gap) * L0, a)),
                           np.sort(rng.uniform(L0 * (1 - half_width), L0 * (1 + half_width), n_shell)),
                           np.sort(rng.uniform((1 + gap) * L0, hi * L0, n - b))])


SMALL_MOTION = (2e-5, -1e-5, 1.5e-5, (2e-4, -3e-4, 2e-4))   # moves no point by 1 % of a designed length
LARGE_MOTION = (2e-3, -1e-3, 1.5e-3, (0.03, -0.02, 0.025))  # iteration 1's cut is > 2 % off the later ones

# name -> (n_src, overlap, max_num_iterations, method, what it is for)
TRIM_CASES = {
    "wide": (12000, 0.5, 6, "pt2pl", "2,000 keys within 1 % of the cut: hit/wide-lds three times, then hit/rank"),
    "sparse": (2000, 0.5, 5, "pt2pl", "about 55 keys in the first window: hit/rank-sparse twice, then hit/rank"),
    "over": (11200, 0.5, 4, "pt2pl", "5,600 keys within 2.2 %: miss/over-4096 (first bin <= 4096), then hit/wide-lds"),
    "global": (16000, 0.5, 4, "pt2pl", "12,000 keys in one first-digit bin: first/global-count, miss/over-4096"),
    "jump": (4000, 0.5, 5, "pt2pl", "two populations and a larger motion: miss/rank-outside, then x4 and hit/rank"),
    "equal": (6000, 0.5, 4, "pt2pl", "400 copies of one source point across the cut: settled in the index bits"),
    "tiny2": (2, 0.5, 4, "pt2pt", "nkeep = 1 of 2"),
    "tiny3": (3, 0.5, 4, "pt2pt", "nkeep = 1 of 3"),
    "tiny33": (33, 0.5, 4, "pt2pt", "nkeep = 16"),
    "tiny64": (64, 0.5, 4, "pt2pt", "one wave exactly"),
    "tiny65": (65, 0.5, 4, "pt2pt", "one wave and a key"),
    "one-of-500": (500, 0.002, 4, "pt2pt", "nkeep = 1 of 500"),
}
# miss/block-over-2048: block 0 of k_trim_window (per = 2560 indices) holds 2,400 in-window keys;
# A1 and the model only on the GPU; left out of the oracle's union, its design checked apart
BLOCK_CASE = (80000, 0.5, 4, "pt2pl")
_PAIRS = {}


def _case(name):
    return BLOCK_CASE if name == "block" else TRIM_CASES[name][:4]


def trim_case_pair(name):
    """(src, tgt) of a designed case, built once and left unchanged."""
    if name in _PAIRS:
        return _PAIRS[name]
    n, overlap, _, method = _case(name)
    seed = 1000 + sorted(list(TRIM_CASES) + ["block"]).index(name)
    rng = np.random.default_rng(seed)
    k = nkeep_of(n, overlap)
    motion = _rigid(*SMALL_MOTION[:3], SMALL_MOTION[3])
    if method == "pt2pt":  # the tiny sources: the first n points of a 3-D lattice, moved in random directions
        tgt = lattice(512, seed)
        v = rng.normal(size=(n, 3))
        v *= (rng.uniform(0.05, 0.3, n) / np.linalg.norm(v, axis=1))[:, None]
        src = _apply(motion, tgt[:n] + v)
    else:
        tgt, axes = corner_planes(n + (1 if name == "equal" else 0), seed)
        by_index = np.empty(n)
        if name == "block":
            per = ((n + 31) // 32 + 63) & ~63
            n_shell = 2400
            assert K_LOC * 1.1 < n_shell <= per - 64
            lens = shell_lengths(n, k, n_shell, 0.003, 0.15, rng)
            a = k - n_shell // 2
            # the shell's ranks on the first indices (k_trim_window's block 0), the others behind
            by_index[rng.permutation(n_shell)] = lens[a:a + n_shell]
            by_index[n_shell + rng.permutation(n - n_shell)] = np.concatenate([lens[:a], lens[a + n_shell:]])
        elif name == "equal":
            # 5,600 distinct points and 400 copies of one more whose length is their median, on
            # shuffled indices: ranks 2800 .. 3199 share their distance bits in every iteration
            nd = n - 400
            dl = np.sort(rng.uniform(0.05, 0.3, nd))
            by_index = np.empty(nd + 1)
            by_index[rng.permutation(nd)] = dl
            by_index[nd] = 0.5 * (dl[nd // 2 - 1] + dl[nd // 2])
        else:
            if name == "wide":
                lens = shell_lengths(n, k, 2000, 0.01, 0.15, rng)
            elif name == "sparse":
                lens = np.sort(rng.uniform(0.05, 0.3, n))
            elif name == "over":  # centred on a first-digit bin edge (0.125): each bin holds half the shell
                lens = shell_lengths(n, k, 5600, 0.022, 0.125, rng)
            elif name == "global":  # [0.127, 0.139] lies inside the bin [0.125, 0.140625)
                lens = shell_lengths(n, k, 12000, 0.045, 0.133, rng, gap=0.15)
            elif name == "jump":
                lens = np.concatenate([np.sort(rng.uniform(0.05, 0.10, k - 10)),
                                       np.sort(rng.uniform(0.2, 0.3, n - k + 10))])
                motion = _rigid(*LARGE_MOTION[:3], LARGE_MOTION[3])
            by_index[rng.permutation(n)] = lens
        src = displaced_source(tgt, axes, by_index, seed + 1, motion)
        if name == "equal":
            src = np.ascontiguousarray(np.concatenate([src[:nd], np.repeat(src[nd:], 400, axis=0)])[rng.permutation(n)])
    assert src.shape == (n, 3)
    src.setflags(write=False)
    tgt.setflags(write=False)
    _PAIRS[name] = (src, tgt)
    return _PAIRS[name]


def _icp_params(overlap, max_iter):
    # mse = 0: `rel < mse` never holds, the run ends at max_num_iterations on both sides
    return dict(estimated_overlap=overlap, max_num_iterations=max_iter, mse=0.0)


_ORACLE = {}


def oracle_run(refcpu, key, pair, rkind, variant, params, margins=True):
    """One oracle run per key, computed once, shared and left unchanged."""
    if key not in _ORACLE:
        ref = refcpu.register(pair[0], pair[1], rkind, variant, refcpu.default_params(**params), trace_iters=160,
                              trace_margins=margins)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _oracle_trim_case(refcpu, name):
    n, overlap, max_iter, method = _case(name)
    return oracle_run(refcpu, ("trim", name), trim_case_pair(name), refcpu.RUN_ICP, method, _icp_params(overlap, max_iter))


def _labels_of_trace(dists, phases, n, overlap):
    return trim_path_model(list(dists), list(phases), n, nkeep_of(n, overlap))


# =========================================================================== A3 on the CPU
def test_model_on_hand_made_keys():
    """The model against windows worked out by hand (n = 4096: per = 128, 32 blocks)."""
    n, k = 4096, 2048
    d0 = np.linspace(1.0, 2.0, n, dtype=np.float32)
    recs = trim_path_model([d0, d0, d0], [2, 2, 2], n, k)
    cut = float(np.sort(d0)[k - 1])
    w0 = np.float32(0.02)
    inside = int(((d0 >= np.float32(cut) * (np.float32(1) - w0)) & (d0 <= np.float32(cut) * (np.float32(1) + w0))).sum())
    assert recs[0]["label"] == "first/compact" and recs[0]["settled"] == "distance"
    assert recs[1]["label"] == "hit/rank" and recs[1]["cnt"] == inside and 96 <= inside <= 768
    assert recs[1]["w"] == pytest.approx(0.02) and recs[2]["w"] == pytest.approx(0.02)
    # a phase change voids the window; all keys equal: one bin of 4096 (still compacted), index bits
    recs = trim_path_model([d0, d0], [1, 2], n, k)
    assert [r["label"] for r in recs] == ["first/compact", "first/compact"]
    recs = trim_path_model([np.ones(n + 1, np.float32)] * 2, [2, 2], n + 1, k)
    assert recs[0]["label"] == "first/global-count" and recs[0]["settled"] == "index"
    assert recs[1]["label"] == "miss/over-4096" and recs[1]["cnt"] == n + 1 and recs[1]["radix"] == "global-count"
    # all of the window in block 0 (indices < 128 ... here per = 2240 for n = 70000)
    n = 70000
    d = np.full(n, 5.0, np.float32)
    d[:2100] = 1.0
    d[2100:30000] = 0.5
    recs = trim_path_model([d, d], [2, 2], n, 29000)
    assert recs[1]["label"] == "miss/block-over-2048" and recs[1]["max_block"] == 2100
    assert recs[1]["cnt"] == K_TRIM_LIST + 1 and recs[1]["below"] == 27900
    # a miss multiplies w by 4, a sparse hit by 1.5, a full window halves it, the cap is 0.9
    d1 = np.linspace(1.0, 2.0, 300, dtype=np.float32)
    recs = trim_path_model([d1 * np.float32(2.0), d1, d1, d1], [2] * 4, 300, 150)
    assert [r["label"] for r in recs] == ["first/compact", "miss/rank-outside", "hit/rank-sparse", "hit/rank"]
    assert [r["w"] for r in recs[1:]] == pytest.approx([0.02, 0.08, 0.12])


def test_nkeep_is_float32_arithmetic():
    assert nkeep_of(3544, 0.9997) == 3542 and nkeep_of(3544, 1.5) == 3544 and nkeep_of(3544, 0.05) == 177
    assert nkeep_of(2, 0.5) == 1 and nkeep_of(3, 0.5) == 1 and nkeep_of(1, 0.7) == 0 and nkeep_of(500, 0.002) == 1
    assert nkeep_of(100, -1.0) == 0


@pytest.mark.parametrize("name", list(TRIM_CASES))
def test_designed_case_labels_have_margin_on_the_oracle(refcpu, name):
    """Every case runs its full number of iterations on the oracle, and no count of the model
    sits within 10 % of 96, 768, 2048 or 4096, so a 1-ulp distance difference between the
    engine and the oracle cannot flip a label."""
    n, overlap, max_iter, method = _case(name)
    ref = _oracle_trim_case(refcpu, name)
    assert ref["num_iterations"] == max_iter >= 4
    recs = _labels_of_trace(ref["corr_dist"][:max_iter], [PHASE_R3] * max_iter, n, overlap)
    print(f"[loop] oracle {name}: {_fmt_labels(recs)}")
    for it, r in enumerate(recs):
        assert not _near_threshold(r), (name, it + 1, r)
    # the design's premise: source i matches target i (duplicates: their original) from iteration 1 on
    if name != "equal":
        assert all(np.array_equal(ref["corr_idx"][it], np.arange(n)) for it in range(max_iter))
    if method == "pt2pl":
        # ... and the pose holds still once the motion is removed: iteration 2 takes out the
        # first step's second-order remainder, later steps are rounding
        step = [float(np.linalg.norm(ref["Ti"][it] - np.eye(4))) for it in range(max_iter)]
        # (quadratic: at most the squared first step times the clouds' half extent, < 50)
        assert step[1] <= 50 * step[0] ** 2 + 1e-9 and max(step[2:]) <= 1e-9, step


def test_designed_cases_reach_every_label_on_the_oracle(refcpu):
    """The union over TRIM_CASES holds every label but miss/block-over-2048 (the 80,000-point
    case is left out of it: test_block_case_design_on_the_oracle) and both settled-by outcomes."""
    seen, settled, by_case = set(), set(), {}
    for name in TRIM_CASES:
        n, overlap, max_iter, _ = _case(name)
        ref = _oracle_trim_case(refcpu, name)
        recs = _labels_of_trace(ref["corr_dist"][:ref["num_iterations"]], [PHASE_R3] * ref["num_iterations"], n, overlap)
        by_case[name] = sorted({r["label"] for r in recs})
        seen |= {r["label"] for r in recs}
        settled |= {r["settled"] for r in recs}
    assert seen == set(LABELS) - {"miss/block-over-2048"}, (sorted(set(LABELS) - seen), by_case)
    assert settled == set(SETTLED)
    # each case reaches what it was designed for
    assert "hit/wide-lds" in by_case["wide"] and "hit/rank" in by_case["wide"]
    assert "hit/rank-sparse" in by_case["sparse"]
    assert "miss/over-4096" in by_case["over"] and "first/compact" in by_case["over"]
    assert "first/global-count" in by_case["global"]
    assert "miss/rank-outside" in by_case["jump"]


def test_block_case_design_on_the_oracle(refcpu):
    """The 80,000-point pair (left out of the union above, as its label comes from the engine's
    own keys on the GPU): the oracle's keys put 2,400 in-window keys into block 0 in every
    windowed iteration, and the rank would have been inside (a hit but for the overflow)."""
    n, overlap, max_iter, _ = _case("block")
    ref = _oracle_trim_case(refcpu, "block")
    recs = _labels_of_trace(ref["corr_dist"][:max_iter], [PHASE_R3] * max_iter, n, overlap)
    assert [r["label"] for r in recs] == ["first/compact"] + ["miss/block-over-2048"] * (max_iter - 1), _fmt_labels(recs)
    k = nkeep_of(n, overlap)
    for r in recs[1:]:
        assert not _near_threshold(r) and r["max_block"] == 2400
        assert r["below"] < k <= r["below"] + 2400 and r["cnt"] == K_TRIM_LIST + 1


# =========================================================================== A3 on the GPU
_GPU = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


def _same_result(a, b):
    return (np.array_equal(_bits(a.T), _bits(b.T)) and a.num_iterations == b.num_iterations and
            a.num_pure_se3_iterations == b.num_pure_se3_iterations and a.status == b.status and
            (a.scaling_factor == b.scaling_factor or (a.scaling_factor != a.scaling_factor and
                                                       b.scaling_factor != b.scaling_factor)))


def _same_trace(a, b):
    return sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def gpu_alone(se3icp_mod, name, max_iter=None):
    """A designed pair registered alone, traced and untraced, once per (case, iteration cap)."""
    n, overlap, mi, method = _case(name)
    mi = mi if max_iter is None else max_iter
    if (name, mi) not in _GPU:
        gp = se3icp_mod.default_params(**_icp_params(overlap, mi))
        pair = trim_case_pair(name)
        res, gtr = se3icp_mod.register_batch_traced([pair], method, gp, pair=0, max_iters=mi + 2)
        plain = se3icp_mod.register_batch([pair], method, gp)[0]
        _GPU[(name, mi)] = (res[0], gtr, plain)
    return _GPU[(name, mi)]


def _check_trim_case(se3icp_mod, name, max_iter=None):
    n, overlap, mi, method = _case(name)
    mi = mi if max_iter is None else max_iter
    g, gtr, plain = gpu_alone(se3icp_mod, name, max_iter)
    assert g.status == 0 and g.num_iterations == mi and len(gtr["phase"]) == mi
    assert set(gtr["phase"].tolist()) == {PHASE_R3} and g.scaling_factor == 1.0
    assert_exact_cut(gtr, n, overlap)
    assert _same_result(plain, g), (name, "untraced run differs", plain.T, g.T)
    return _labels_of_trace(gtr["corr_dist"], gtr["phase"], n, overlap)


@gpu
@pytest.mark.parametrize("name", list(TRIM_CASES) + ["block"])
def test_exact_cut_on_designed_keys(se3icp_mod, refcpu, parity_record, name):
    """A1 on a designed pair, the untraced run bitwise equal, and the engine's own keys take
    the paths the oracle's do (the counts keep 10 % from every threshold, and the two sides'
    distances differ by at most 1 ulp).  Against the oracle: compare_traces, nothing excused."""
    from test_gpu_trace import compare_traces
    n, overlap, max_iter, method = _case(name)
    recs = _check_trim_case(se3icp_mod, name)
    print(f"[loop] engine {name}: {_fmt_labels(recs)}")
    for it, r in enumerate(recs):
        assert not _near_threshold(r), (name, it + 1, r)
    g, gtr, _ = gpu_alone(se3icp_mod, name)
    counters = dict(n_src=n, nkeep=nkeep_of(n, overlap), labels=[r["label"] for r in recs],
                    settled=[r["settled"] for r in recs], window_counts=[r.get("cnt") for r in recs])
    if name != "block":
        ref = _oracle_trim_case(refcpu, name)
        assert g.num_iterations == ref["num_iterations"]
        want = _labels_of_trace(ref["corr_dist"][:max_iter], [PHASE_R3] * max_iter, n, overlap)
        assert [r["label"] for r in recs] == [r["label"] for r in want], (_fmt_labels(recs), _fmt_labels(want))
        tot = compare_traces(gtr, ref, overlap, "loop: " + name)
        assert tot["idx_diff"] == 0, tot
        counters.update(dist_ulp1=tot["dist_ulp1"], kept_swaps=tot["kept_swaps"], max_pose_diff=tot["max_pose_diff"])
    else:
        assert [r["label"] for r in recs] == ["first/compact"] + ["miss/block-over-2048"] * (max_iter - 1)
    parity_record("loop: trim " + name, **counters)


@gpu
def test_every_trim_path_is_reached_on_the_engine(se3icp_mod):
    """The condition that keeps A1 honest: over the designed cases the engine's own keys take
    every path of LABELS and settle the cut both ways."""
    seen, settled, by_case = set(), set(), {}
    for name in list(TRIM_CASES) + ["block"]:
        _, gtr, _ = gpu_alone(se3icp_mod, name)
        n, overlap, _, _ = _case(name)
        recs = _labels_of_trace(gtr["corr_dist"], gtr["phase"], n, overlap)
        by_case[name] = sorted({r["label"] for r in recs})
        seen |= {r["label"] for r in recs}
        settled |= {r["settled"] for r in recs}
    assert seen == set(LABELS), (sorted(set(LABELS) - seen), by_case)
    assert settled == set(SETTLED)
    # the radix select under a miss took both of its paths too
    radix = set()
    for name in ("over", "global", "jump"):
        _, gtr, _ = gpu_alone(se3icp_mod, name)
        n, overlap, _, _ = _case(name)
        radix |= {(r["label"].split("/")[0], r["radix"]) for r in _labels_of_trace(gtr["corr_dist"], gtr["phase"], n, overlap)
                  if r["radix"]}
    assert {("miss", "compact"), ("miss", "global-count"), ("first", "compact"), ("first", "global-count")} <= radix, radix


@gpu
def test_keep_none_against_the_oracle(se3icp_mod, refcpu, parity_record):
    """estimated_overlap = 0: nkeep = 0, nothing is kept (k_trim writes no cut, k_reduce sums
    nothing).  Both sides run to max_num_iterations = 3, leave the pose alone and report the
    mean of no distances as NaN."""
    src, tgt = trim_case_pair("one-of-500")
    params = dict(estimated_overlap=0.0, max_num_iterations=3)
    ref = oracle_run(refcpu, ("keep-none",), (src, tgt), refcpu.RUN_ICP, "pt2pt", params)
    gp = se3icp_mod.default_params(**params)
    res, gtr = se3icp_mod.register_batch_traced([(src, tgt)], "pt2pt", gp, pair=0, max_iters=8)
    g = res[0]
    assert ref["num_iterations"] == 3 and g.num_iterations == 3 and len(gtr["phase"]) == 3
    assert (ref["n_kept"][:3] == 0).all()
    assert np.array_equal(ref["T"], np.eye(4)) and np.array_equal(g.T, np.eye(4))
    assert all(np.array_equal(gtr["T"][it], np.eye(4)) for it in range(3))
    assert np.isnan(ref["mse"][:3]).all() and np.isnan(gtr["mse"]).all()
    assert_exact_cut(gtr, src.shape[0], 0.0)
    assert np.array_equal(gtr["corr_idx"][0], ref["corr_idx"][0])
    plain = se3icp_mod.register_batch([(src, tgt)], "pt2pt", gp)[0]
    assert _same_result(plain, g)
    parity_record("loop: keep none", iterations=3, mse_is_nan=True)


# --------------------------------------------------------------------------- A1 on existing-style runs
def _pair_b(bunny_unique):
    from se3icp import datasets
    src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=2, subsample=0.1)
    assert (src.shape[0], tgt.shape[0]) == (3544, 3563)
    return src, tgt


_KITTI = {}


def _kitti_scans():
    """One KITTI-like pair of ~120k-point scans (source = scan 6, target = scan 5), cast once."""
    if not _KITTI:
        from se3icp import datasets
        pairs, _ = datasets.kitti_like_pairs(1, seed=4, first=5, total_pairs=8)
        _KITTI["scans"] = pairs[0]
    return _KITTI["scans"]


def _kitti_sub(n_src, n_tgt, seed=16):
    src, tgt = _kitti_scans()
    rng = np.random.default_rng(seed)
    s = src[np.sort(rng.choice(len(src), n_src, replace=False))]
    t = tgt[np.sort(rng.choice(len(tgt), n_tgt, replace=False))]
    return np.ascontiguousarray(s), np.ascontiguousarray(t)


B_PARAMS = dict(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-5, mse_switch_error=5e-5,
                number_of_nn_for_LRF=60)
R_PARAMS = dict(estimated_overlap=0.75, max_num_se3_iterations=10, mse_switch_error=5e-5, number_of_nn_for_LRF=90)
K_PARAMS = dict(estimated_overlap=0.7, max_num_se3_iterations=10, mse=1e-7, mse_switch_error=5e-7,
                number_of_nn_for_LRF=90)


@gpu
@pytest.mark.parametrize("case", ["bunny se3_pt2pt 0.5", "rgbd cf 0.75", "kitti16k se3_gicp 0.7"])
def test_exact_cut_on_end_to_end_runs(se3icp_mod, bunny_unique, parity_record, case):
    """A1 where the keys come from real searches in both phases: the SE(3) -> R3 switch voids
    the window mid-run (the R3 cut is far below the SE(3) one)."""
    if case.startswith("bunny"):
        pair, method, params = _pair_b(bunny_unique), "se3_pt2pt", dict(B_PARAMS, estimated_overlap=0.5)
    elif case.startswith("rgbd"):
        from se3icp import datasets
        pair, method, params = datasets.rgbd_pairs(1, seed=5, stride=8)[0][0], "se3_gicp_with_cf", R_PARAMS
    else:
        pair, method, params = _kitti_sub(16000, 16000), "se3_gicp", K_PARAMS
    res, gtr = se3icp_mod.register_batch_traced([pair], method, se3icp_mod.default_params(**params), pair=0, max_iters=160)
    g = res[0]
    assert g.status == 0 and len(gtr["phase"]) == g.num_iterations
    n = pair[0].shape[0]
    assert_exact_cut(gtr, n, params["estimated_overlap"])
    phases = gtr["phase"].tolist()
    assert phases == [PHASE_SE3] * g.num_pure_se3_iterations + [PHASE_R3] * (g.num_iterations - g.num_pure_se3_iterations)
    assert 0 < g.num_pure_se3_iterations < g.num_iterations
    recs = _labels_of_trace(gtr["corr_dist"], phases, n, params["estimated_overlap"])
    print(f"[loop] engine {case}: {_fmt_labels(recs)}")
    sw = g.num_pure_se3_iterations
    assert recs[0]["label"].startswith("first/") and recs[sw]["label"].startswith("first/")
    assert all(not r["label"].startswith("first/") for i, r in enumerate(recs) if i not in (0, sw))
    parity_record("loop: cut " + case, iterations=int(g.num_iterations), pure_se3_iterations=int(sw),
                  labels=[r["label"] for r in recs])


# =========================================================================== A4: batches and scratch
BATCH = ["wide", "sparse", "over", "jump", "equal"]
BATCH_ITERS = 5
SMALL_BATCH = ["global", "sparse"]


@gpu
def test_batched_pairs_equal_the_pairs_alone(se3icp_mod):
    """Five designed pairs of different sizes and paths in one batch, traced once per pair index:
    A1 holds, and the trace and the result are bitwise those of the pair run alone."""
    gp = se3icp_mod.default_params(**_icp_params(0.5, BATCH_ITERS))
    pairs = [trim_case_pair(name) for name in BATCH]
    assert len({p[0].shape[0] for p in pairs}) == len(BATCH)
    paths = set()
    for k, name in enumerate(BATCH):
        recs = _check_trim_case(se3icp_mod, name, BATCH_ITERS)
        paths |= {r["label"] for r in recs}
        _, alone_tr, _ = gpu_alone(se3icp_mod, name, BATCH_ITERS)
        res, gtr = se3icp_mod.register_batch_traced(pairs, "pt2pl", gp, pair=k, max_iters=BATCH_ITERS + 2)
        assert_exact_cut(gtr, pairs[k][0].shape[0], 0.5)
        assert _same_trace(gtr, alone_tr), (name, [key for key in gtr if not np.array_equal(_bits(gtr[key]), _bits(alone_tr[key]))])
        for j, other in enumerate(BATCH):
            assert _same_result(res[j], gpu_alone(se3icp_mod, other, BATCH_ITERS)[0]), (name, other)
    assert {"first/compact", "hit/rank", "hit/rank-sparse", "hit/wide-lds", "miss/rank-outside", "miss/over-4096"} <= paths


@gpu
def test_scratch_is_reset_across_batches_of_different_sizes(se3icp_mod):
    """trim_ctr, trim_hist, trim_cand and the window word live per pair slot and are reset by
    whichever path ran last: a 5-pair batch, a 2-pair batch whose slots 0 and 1 held other
    pairs (and whose last iterations took other paths), and both again, on one engine.  Every
    run is bitwise its first run and the pairs run alone."""
    gp = se3icp_mod.default_params(**_icp_params(0.5, BATCH_ITERS))
    big = [trim_case_pair(name) for name in BATCH]
    small = [trim_case_pair(name) for name in SMALL_BATCH]
    first_big = se3icp_mod.register_batch(big, "pt2pl", gp)
    first_small = se3icp_mod.register_batch(small, "pt2pl", gp)
    for rep in range(2):
        again_big = se3icp_mod.register_batch(big, "pt2pl", gp)
        again_small = se3icp_mod.register_batch(small, "pt2pl", gp)
        assert all(_same_result(a, b) for a, b in zip(again_big, first_big)), rep
        assert all(_same_result(a, b) for a, b in zip(again_small, first_small)), rep
    for name, r in list(zip(BATCH, first_big)) + list(zip(SMALL_BATCH, first_small)):
        assert _same_result(r, gpu_alone(se3icp_mod, name, BATCH_ITERS)[0]), name


# =========================================================================== A5: sums and solve
LD = np.longdouble
SUM_SIZES = [1, 255, 256, 257, 32256, 32257, 36864, 36865, 69120, 69121]  # 126|127, 144|145, 270|271 blocks of 256
SUM_OVERLAPS = [1.0, 0.7]
SUM_TARGET = 8000
SUM_ITERS = 3
SUM_MOTION = (0.01, -0.008, 0.012, (0.05, -0.04, 0.03))
NORMAL_SIZES = [32257, 36865]


def sums_pair(n):
    """n source points around random points of an 8,000-point lattice target, then moved."""
    key = ("sums", n)
    if key not in _PAIRS:
        tgt = lattice(SUM_TARGET, 77)
        rng = np.random.default_rng(5000 + n)
        v = rng.normal(size=(n, 3))
        v *= (rng.uniform(0.02, 0.25, n) / np.linalg.norm(v, axis=1))[:, None]
        src = _apply(_rigid(*SUM_MOTION[:3], SUM_MOTION[3]), tgt[rng.integers(0, SUM_TARGET, n)] + v)
        src.setflags(write=False)
        tgt.setflags(write=False)
        _PAIRS[key] = (src, tgt)
    return _PAIRS[key]


def _inv3_ld(m):
    c = np.empty((3, 3), LD)
    c[0, 0] = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c[0, 1] = m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]
    c[0, 2] = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
    c[1, 0] = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c[1, 1] = m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]
    c[1, 2] = m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]
    c[2, 0] = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    c[2, 1] = m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]
    c[2, 2] = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    return c / (m[0, 0] * c[0, 0] + m[0, 1] * c[1, 0] + m[0, 2] * c[2, 0])


def _umeyama_rotation_ld(sigma):
    """Eigen::umeyama's R = U S V^T of the long-double sigma.  For a well-conditioned sigma
    of positive determinant that is its orthogonal polar factor, taken in long double by
    Newton's iteration X <- (X + X^-T) / 2 from X = sigma; otherwise (reflection, rank
    deficiency) the f64 SVD; a zero sigma gives the identity (JacobiSVD: U = V = I)."""
    s64 = sigma.astype(np.float64)
    if not s64.any():
        return np.eye(3, dtype=LD)
    U, sv, Vt = np.linalg.svd(s64)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R0 = (U @ S @ Vt).astype(LD)
    if S[2, 2] < 0 or sv[2] < 1e-3 * sv[0]:
        return R0
    X = sigma / LD(sv[0])
    for _ in range(60):
        Xn = (X + _inv3_ld(X).T) / LD(2)
        done = float(np.abs(Xn - X).max()) < 1e-18
        X = Xn
        if done:
            break
    assert float(np.abs(X - R0).max()) < 1e-10
    return X


def umeyama_ld(vs, vt):
    """Two-pass, centred Eigen::umeyama(vs, vt, false) in long double: 4 x 4."""
    T = np.eye(4, dtype=LD)
    K = vs.shape[0]
    if K == 0:
        return T
    ms, md = vs.sum(0) / LD(K), vt.sum(0) / LD(K)
    sigma = (vt - md).T @ (vs - ms) / LD(K)
    R = _umeyama_rotation_ld(sigma)
    T[:3, :3] = R
    T[:3, 3] = md - R @ ms
    return T


def step_deviation(src, tgt, corr_idx, corr_dist, T_acc, mse, overlap):
    """Every iteration of a pt2pt run recomputed from its trace alone.  Iteration it keeps the
    keys up to the nkeep-th smallest (all when nothing is trimmed), and then
        vs = T[it-1] src (T[-1] = I), vt = tgt[corr_idx[it]],
        mse[it] = sum of the kept float distances / K,  T[it] = umeyama(vs, vt) T[it-1].
    Returns (largest |T[it] - recomputed|_F, largest |mse[it] - recomputed| / recomputed,
    largest |T|_F); with nothing kept the pose must stay bitwise and the mse be NaN."""
    n = src.shape[0]
    k = nkeep_of(n, overlap)
    src_ld, tgt_ld = src.astype(LD), tgt.astype(LD)
    dev_T, dev_mse, norm_T = 0.0, 0.0, 1.0
    for it in range(len(corr_idx)):
        Tp = np.eye(4) if it == 0 else T_acc[it - 1]
        if k >= n:
            kept = np.arange(n)
        elif k <= 0:
            assert np.array_equal(T_acc[it], Tp) and np.isnan(mse[it])
            continue
        else:
            keys = trim_keys(corr_dist[it])
            kept = np.nonzero(keys <= np.sort(keys)[k - 1])[0]
            assert kept.shape[0] == k
        Tp = Tp.astype(LD)
        vs = src_ld[kept] @ Tp[:3, :3].T + Tp[:3, 3]
        vt = tgt_ld[corr_idx[it][kept]]
        want_T = umeyama_ld(vs, vt) @ Tp
        want_mse = corr_dist[it][kept].astype(LD).sum() / LD(kept.shape[0])
        dev_T = max(dev_T, float(np.sqrt(((T_acc[it].astype(LD) - want_T) ** 2).sum())))
        if want_mse > 0:
            dev_mse = max(dev_mse, float(abs(LD(mse[it]) - want_mse) / want_mse))
        else:  # (a single kept point, aligned exactly by the step before)
            assert mse[it] == 0.0
        norm_T = max(norm_T, float(np.linalg.norm(T_acc[it])))
    return dev_T, dev_mse, norm_T


def _sum_params(overlap):
    return dict(estimated_overlap=overlap, max_num_iterations=SUM_ITERS, mse=0.0)


_ORACLE_DEV = {}


def oracle_step_deviation(refcpu, n, overlap):
    """The oracle's own est_pt2pt / mse (f64, centred, 64 chunks summed in order) against the
    long-double recompute of its own trace, once per case."""
    if (n, overlap) not in _ORACLE_DEV:
        src, tgt = sums_pair(n)
        ref = oracle_run(refcpu, ("sums", n, overlap), (src, tgt), refcpu.RUN_ICP, "pt2pt", _sum_params(overlap), margins=False)
        n_it = ref["num_iterations"]
        T_acc, T = [], np.eye(4)
        for it in range(n_it):
            T = ref["Ti"][it] @ T
            T_acc.append(T)
        _ORACLE_DEV[(n, overlap)] = (ref, step_deviation(src, tgt, ref["corr_idx"][:n_it], ref["corr_dist"][:n_it], T_acc,
                                                         ref["mse"][:n_it], overlap))
    return _ORACLE_DEV[(n, overlap)]


def _mse_bar(n):
    # any order of summing K <= n non-negative f64 terms is within (K - 1) 2^-53 of the exact
    # sum, relative; the division adds one rounding
    return n * 2.0 ** -53


@pytest.mark.parametrize("overlap", SUM_OVERLAPS)
@pytest.mark.parametrize("n", SUM_SIZES)
def test_oracle_step_deviation_from_long_double(refcpu, n, overlap):
    """What the engine's bar is made of: the oracle runs SUM_ITERS iterations and its own steps
    stay within 1e-12 |T| of the long-double recompute (a centred f64 umeyama of a
    well-conditioned cloud carries a few hundred eps at most; a larger figure would make
    10 x it a vacuous bar)."""
    ref, (dev_T, dev_mse, norm_T) = oracle_step_deviation(refcpu, n, overlap)
    print(f"[loop] oracle sums n {n} overlap {overlap}: |T - T_ld|_F {dev_T:.2e}, mse {dev_mse:.2e} relative")
    assert ref["num_iterations"] == SUM_ITERS
    assert dev_T <= 1e-12 * norm_T, (n, overlap, dev_T)
    assert dev_mse <= _mse_bar(n), (n, overlap, dev_mse)


@gpu
@pytest.mark.parametrize("overlap", SUM_OVERLAPS)
@pytest.mark.parametrize("n", SUM_SIZES)
def test_pt2pt_step_recomputed_from_the_trace(se3icp_mod, refcpu, parity_record, n, overlap):
    """k_reduce's pt2pt sums, k_reduce_final's chains and the solve at the reduction's
    structural sizes: every iteration's pose within 10 x the oracle's largest deviation from
    the same long-double recompute (the factor covers the different summation trees; floor
    1e-13 max(1, |T|)), its MSE within the bound of any summation order, A1, and the untraced
    run bitwise equal."""
    src, tgt = sums_pair(n)
    ref, (ref_T, ref_mse, _) = oracle_step_deviation(refcpu, n, overlap)
    gp = se3icp_mod.default_params(**_sum_params(overlap))
    res, gtr = se3icp_mod.register_batch_traced([(src, tgt)], "pt2pt", gp, pair=0, max_iters=SUM_ITERS + 2)
    g = res[0]
    assert g.status == 0 and g.num_iterations == ref["num_iterations"] == SUM_ITERS == len(gtr["phase"])
    assert_exact_cut(gtr, n, overlap)
    dev_T, dev_mse, norm_T = step_deviation(src, tgt, gtr["corr_idx"], gtr["corr_dist"], gtr["T"], gtr["mse"], overlap)
    bar = max(10 * ref_T, 1e-13 * norm_T)
    print(f"[loop] engine sums n {n} overlap {overlap}: |T - T_ld|_F {dev_T:.2e} (oracle {ref_T:.2e}, bar {bar:.2e}), "
          f"mse {dev_mse:.2e} (oracle {ref_mse:.2e}, bar {_mse_bar(n):.2e})")
    parity_record(f"loop: pt2pt step n={n} overlap={overlap}", blocks=(n + 255) // 256, oracle_pose_dev=ref_T,
                  engine_pose_dev=dev_T, pose_bar=bar, oracle_mse_dev=ref_mse, engine_mse_dev=dev_mse, mse_bar=_mse_bar(n))
    assert dev_T <= bar, (n, overlap, dev_T, bar)
    assert dev_mse <= _mse_bar(n), (n, overlap, dev_mse)
    assert np.array_equal(gtr["corr_idx"][0], ref["corr_idx"][0])
    plain = se3icp_mod.register_batch([(src, tgt)], "pt2pt", gp)[0]
    assert _same_result(plain, g)


def normals_pair(n):
    """n source points of one KITTI-like scan against 8,000 of the previous one."""
    key = ("normals", n)
    if key not in _PAIRS:
        _PAIRS[key] = _kitti_sub(n, SUM_TARGET, seed=n)
    return _PAIRS[key]


@gpu
@pytest.mark.parametrize("variant", ["pt2pl", "gicp"])
@pytest.mark.parametrize("n", NORMAL_SIZES)
def test_jacobian_sums_at_the_reduction_edges(se3icp_mod, refcpu, parity_record, n, variant):
    """pt2pl and gicp at 127 and 145 blocks (the first trip of k_reduce_final's unrolled loop
    with one chain short, and past it), against the oracle through compare_traces: every index
    difference an excused near-tie, poses within 1e-9."""
    from test_gpu_trace import compare_traces
    pair = normals_pair(n)
    params = dict(estimated_overlap=0.7, max_num_iterations=SUM_ITERS, mse=0.0)
    ref = oracle_run(refcpu, ("normals", n, variant), pair, refcpu.RUN_ICP, variant, params)
    res, gtr = se3icp_mod.register_batch_traced([pair], variant, se3icp_mod.default_params(**params), pair=0,
                                                max_iters=SUM_ITERS + 2)
    g = res[0]
    assert g.status == 0 and g.num_iterations == ref["num_iterations"] == SUM_ITERS
    assert_exact_cut(gtr, n, 0.7)
    tot = compare_traces(gtr, ref, 0.7, f"loop: {variant} n={n}")
    assert np.linalg.norm(g.T - ref["T"]) <= 1e-5
    parity_record(f"loop: {variant} n={n}", blocks=(n + 255) // 256, idx_diff=tot["idx_diff"], dist_ulp1=tot["dist_ulp1"],
                  kept_swaps=tot["kept_swaps"], max_pose_diff=tot["max_pose_diff"])
    plain = se3icp_mod.register_batch([pair], variant, se3icp_mod.default_params(**params))[0]
    assert _same_result(plain, g)


# =========================================================================== A6: away from the origin
# Translation equivariance: registering (src + c, tgt + c) must give S(c) T0 S(-c), where T0
# registers (src, tgt) and S(c) translates by c.  run_icp works in raw coordinates, so a scan
# in UTM coordinates (|c| / spread ~ 1e5) puts the estimators' cancellations to the test; the
# run_se3_* methods normalize first.
#
# The reference's pt2pl and gicp steps are Gauss-Newton steps in the angles of a rotation about
# the origin (TransformVector6dToMatrix4d), so those two methods are not equivariant by
# construction: away from the origin the linearization carries a lever arm |c|, the iterations
# take another path and, far enough out, diverge.  The oracle, on the CPU, with these clouds:
#   bunny (3.5k points, spread 2.9, 45-degree initial error) pt2pl: 47 iterations unshifted, 40 / 41 /
#     35 at shifts of 1e1 / 1e2 / 1e3 (0.6, -0.7, 0.4), defects 1.5e-4 / 1.8e-3 / 3e19; gicp 24
#     against 21 / 31 / 150, defects 6e-3 / 1.0 / 6.9; at 1e4: 150 iterations, 5e116 and 20;
#   kitti16k (spread 15, 1 m between the scans) pt2pl: 26 iterations unshifted, 26 / 25 / 28 / 13 at
#     1e2 / 1e3 / 1e4 / 1e5, defects 4e-14 / 2e-6 / 8e-10 / 3e17, and 15 iterations, 8e26 at the
#     UTM offset; gicp: 150 iterations everywhere, defects 2e-13 / 4e-11 / 2e-9 / 8.2 and 10.3.
# A case is kept only where the oracle runs the same number of iterations on both inputs and
# ends at the same alignment, which leaves, of pt2pl and gicp, the KITTI-like pair at 1e2 and
# 1e4; pt2pt (umeyama is equivariant) and the normalizing run_se3_* stay at the full offsets.
SHIFT_DIR = np.array([0.6, -0.7, 0.4])
SHIFTS = {"1e2": 1e2 * SHIFT_DIR, "1e4": 1e4 * SHIFT_DIR, "utm": np.array([4.1e5, 5.5e6, 120.0])}
OFF_CASES = [("bunny", "pt2pt", "1e4"), ("bunny", "se3_pt2pt", "1e4"),
             ("kitti16k", "pt2pt", "utm"), ("kitti16k", "se3_gicp", "utm"),
             ("kitti16k", "pt2pl", "1e2"), ("kitti16k", "gicp", "1e4")]


def _off_case(bunny_unique, cloud, method, where):
    if cloud == "bunny":
        pair, params = _pair_b(bunny_unique), B_PARAMS
    else:
        pair, params = _kitti_sub(16000, 16000), K_PARAMS
    shift = SHIFTS[where]
    key = ("off", cloud, where)
    if key not in _PAIRS:
        _PAIRS[key] = (np.ascontiguousarray(pair[0] + shift), np.ascontiguousarray(pair[1] + shift))
    return pair, _PAIRS[key], shift, params


def _conjugate_ld(T, c):
    """S(c) T S(-c) in long double: the same rotation, t + c - R c."""
    T, c = T.astype(LD), np.asarray(c).astype(LD)
    out = T.copy()
    out[:3, 3] = T[:3, 3] + c - T[:3, :3] @ c
    return out


def pose_gap(Ta, Tb, pts):
    """The largest displacement of a point of pts between the poses Ta and Tb over the spread
    of pts (root mean square distance from their centroid), in long double."""
    p, Ta, Tb = pts.astype(LD), Ta.astype(LD), Tb.astype(LD)
    d = p @ (Ta[:3, :3] - Tb[:3, :3]).T + (Ta[:3, 3] - Tb[:3, 3])
    spread = np.sqrt(((p - p.mean(0)) ** 2).sum(1).mean())
    return float(np.sqrt((d ** 2).sum(1).max()) / spread)


def _oracle_off(refcpu, bunny_unique, cloud, method, where):
    """The oracle on the unshifted and the shifted input, and its own equivariance defect."""
    pair, shifted, shift, params = _off_case(bunny_unique, cloud, method, where)
    se3 = method.startswith("se3_")
    rkind, variant = (refcpu.RUN_SE3_ICP if se3 else refcpu.RUN_ICP), method.replace("se3_", "")
    r0 = oracle_run(refcpu, ("off0", cloud, method), pair, rkind, variant, params, margins=False)
    r1 = oracle_run(refcpu, ("off1", cloud, method, where), shifted, rkind, variant, params, margins=False)
    d_ref = pose_gap(r1["T"], _conjugate_ld(r0["T"], shift), shifted[0])
    return r0, r1, d_ref


@pytest.mark.parametrize("cloud,method,where", OFF_CASES)
def test_oracle_is_translation_equivariant(refcpu, bunny_unique, cloud, method, where):
    """A case is kept only if the oracle runs the same number of iterations on both inputs (a
    pair whose stopping test is decided by rounding cannot carry a bar); its defect d_ref is
    then the conditioning the reference itself shows, and sets the engine's bar."""
    r0, r1, d_ref = _oracle_off(refcpu, bunny_unique, cloud, method, where)
    print(f"[off] oracle {cloud} {method} at {where}: iterations {r0['num_iterations']}/{r0['num_pure_se3_iterations']} unshifted, "
          f"{r1['num_iterations']}/{r1['num_pure_se3_iterations']} shifted, defect {d_ref:.3e}")
    assert (r0["num_iterations"], r0["num_pure_se3_iterations"]) == (r1["num_iterations"], r1["num_pure_se3_iterations"])
    assert d_ref < 1e-3  # the two runs found the same alignment


@gpu
@pytest.mark.parametrize("cloud,method,where", OFF_CASES)
def test_registration_away_from_the_origin(se3icp_mod, refcpu, bunny_unique, parity_record, cloud, method, where):
    """The engine on the shifted input against the oracle on the same input: equal iteration
    counts, and the pose within max(10 x the oracle's own equivariance defect, the suite's
    end-to-end bar |T_gpu - T_ref|_F <= 1e-5 taken in a frame re-centred on the target
    centroid, where it means what it means for the other tests' clouds).

    Before the pt2pt moments were taken about a pivot (k_loop.hip corr_terms) the engine ran the
    KITTI-like pair at the UTM offset for 43 iterations against the oracle's 38 and ended 1.8e-3
    spreads away (re-centred |T_gpu - T_ref|_F 9.6e-4); on the bunny at 1e4 it ended 8.5e-9
    spreads away, 5,600 times the oracle's defect though within the 1e-5 bar, which is why the
    pt2pt cases also hold the engine's own equivariance defect to 10 x the oracle's."""
    pair, shifted, shift, params = _off_case(bunny_unique, cloud, method, where)
    _, r1, d_ref = _oracle_off(refcpu, bunny_unique, cloud, method, where)
    g = se3icp_mod.register_batch([shifted], method, se3icp_mod.default_params(**params))[0]
    gap = pose_gap(g.T, r1["T"], shifted[0])
    ct = shifted[1].mean(0)
    recentred = float(np.sqrt(((_conjugate_ld(g.T, -ct) - _conjugate_ld(r1["T"], -ct)) ** 2).sum()))
    print(f"[off] engine {cloud} {method} at {where}: iterations {g.num_iterations}/{g.num_pure_se3_iterations} oracle "
          f"{r1['num_iterations']}/{r1['num_pure_se3_iterations']}, gap {gap:.3e}, oracle defect {d_ref:.3e}, "
          f"re-centred |T_gpu - T_ref|_F {recentred:.3e}")
    parity_record(f"loop: off-origin {cloud} {method} at {where}", shift_over_spread=float(np.linalg.norm(shift) / np.sqrt(
        ((shifted[0] - shifted[0].mean(0)) ** 2).sum(1).mean())), oracle_defect=d_ref, engine_gap=gap,
        recentred_pose_diff=recentred, iterations=int(g.num_iterations))
    assert g.status == 0
    assert g.num_iterations == r1["num_iterations"], (g.num_iterations, r1["num_iterations"])
    if method.startswith("se3_"):
        assert g.num_pure_se3_iterations == r1["num_pure_se3_iterations"]
    assert gap <= 10 * d_ref or recentred <= 1e-5, (cloud, method, where, gap, d_ref, recentred)
    if method == "pt2pt":
        # umeyama is equivariant in exact arithmetic, so the engine's own defect (its run on the
        # unshifted pair, conjugated) is rounding alone, like the oracle's: within 10 x d_ref
        g0 = se3icp_mod.register_batch([pair], method, se3icp_mod.default_params(**params))[0]
        own = pose_gap(g.T, _conjugate_ld(g0.T, shift), shifted[0])
        print(f"[off] engine {cloud} {method} at {where}: own equivariance defect {own:.3e}")
        parity_record(f"loop: off-origin {cloud} {method} at {where}", engine_own_defect=own)
        assert g0.num_iterations == g.num_iterations and own <= 10 * d_ref, (cloud, where, own, d_ref)
