"""Designed inputs, a long-double brute force and the checker of the NN certificate tests (DESIGN
section 23): tests/test_gpu_certificates.py runs the engine's se3icp_nn_sequence through `check_run`,
tests/test_cert_host.py runs numpy models of the certificates through the same checker -- an exact
one (the design figures) and a restatement of csrc/nn_cert.hpp with planted defects (the checker can
fail).

A case is a dict: dim, alpha, query (nq, dim), data (nd, dim), poses (n_steps, 4, 4), restart_at.
Step k (1-based) is iteration k: the query is poses[k - 1] applied to its row (a point, or a
frame [alpha x | alpha y | alpha z | t] in the packing of the engine's 12-vectors)."""
import functools

import numpy as np

from tree_cases import inflation_fused

LD = np.longdouble
EPS = 2.0 ** -52
K_HIST = 256          # pose ring of the loop (csrc/common.hpp kHist)
K_SHORT = 8           # candidates per query resolved in long double
U32 = np.float32(5.9604645e-08)


# ------------------------------------------------------------------ poses
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def exp_se3(w, t):
    """exp of the twist (w, t) as a 4x4 (Rodrigues; series below 1e-4 rad)."""
    th = float(np.linalg.norm(w))
    K = hat(w)
    if th < 1e-4:
        a, b, c = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0, 1.0 / 6.0 - th * th / 120.0
    else:
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * (K @ K)
    T[:3, 3] = (np.eye(3) + b * K + c * (K @ K)) @ t
    return T


def twist_poses(w, t, rho, n_steps):
    """T_k = exp(rho^(k-1) (w, t)), k = 1 .. n_steps: the geometric decay of a converging run."""
    return np.stack([exp_se3(rho ** k * w, rho ** k * t) for k in range(n_steps)])


def apply_pose(T, M, dim, dtype=LD):
    """The queries T * M0 (rows of M) in `dtype`: pose_point / pose_frame evaluated exactly enough."""
    T = np.asarray(T, dtype)
    M = np.asarray(M, dtype)
    R, t = T[:3, :3], T[:3, 3]
    if dim == 3:
        return M @ R.T + t
    out = np.empty_like(M)
    for c in range(3):
        out[:, 3 * c:3 * c + 3] = M[:, 3 * c:3 * c + 3] @ R.T
    out[:, 9:12] = M[:, 9:12] @ R.T + t
    return out


# ------------------------------------------------------------------ designed inputs
def _unit(rng, n, d):
    v = rng.standard_normal((n, d))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def aligned_case(dim, n, alpha=1.0, seed=1, delta=0.02, rho=0.6, steps=30, w0=0.27, t0=0.07, scale=1.0,
                 restart_at=0, shuffle=True):
    """"Aligned pairs": query i moves, late in the run, along u_i ~ xi * M0_i; two targets sit on
    that line on opposite sides of it (at delta and delta (1 + eps_i), eps log-uniform in [1e-9, 0.3]),
    so a displacement dl changes d2 - d1 by exactly 2 dl and the arg-min flips just where a sound
    certificate must refuse to settle; a third at delta (1 + eta_i), eta log-uniform in [1e-7, 3],
    in a random direction (either side of the widened pruning radius)."""
    rng = np.random.default_rng(seed)
    w = _unit(rng, 1, 3)[0] * w0
    t = _unit(rng, 1, 3)[0] * t0 * scale
    p = _unit(rng, n, 3) * rng.uniform(0, 1, (n, 1)) ** (1.0 / 3.0) * scale
    if dim == 3:
        M0 = p
        u = np.cross(w, p) + t
    else:
        X = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]          # columns orthonormal to rounding
        M0 = np.concatenate([alpha * X[:, :, c] for c in range(3)] + [p], axis=1)
        u = np.concatenate([alpha * np.cross(w, X[:, :, c]) for c in range(3)] + [np.cross(w, p) + t], axis=1)
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    s = rng.choice([-1.0, 1.0], (n, 1))
    eps = _log_uniform(rng, 1e-9, 0.3, n)[:, None]
    eta = _log_uniform(rng, 1e-7, 3.0, n)[:, None]
    data = np.concatenate([M0 + s * delta * u, M0 - s * delta * (1.0 + eps) * u,
                           M0 + delta * (1.0 + eta) * _unit(rng, n, dim)])
    if shuffle:
        data = data[rng.permutation(len(data))]
    return dict(dim=dim, alpha=float(alpha), query=np.ascontiguousarray(M0), data=np.ascontiguousarray(data),
                poses=twist_poses(w, t, rho, steps), restart_at=restart_at)


# the cases of the GPU tests (and of the CPU design tests): name -> builder
N_MAIN = 600


def main_cases():
    c = {"r3": lambda: aligned_case(3, N_MAIN, seed=11)}
    for a, d in ((0.0, 0.02), (0.3, 0.02), (3.0, 0.02), (1000.0, 0.02 * 1000.0 / 3.0)):
        # (alpha 1000: the queries move ~alpha / 3 times as far per step; delta scales with it)
        c["se3_a%g" % a] = functools.partial(aligned_case, 12, N_MAIN, alpha=a, seed=12, delta=d)
    # alpha 0 with a larger twist: a one-pair SE(3) run widens its searches from iteration 4 on
    # (k_nn.hip widen_from), so the engine settles nothing before step 5; with the base twist the
    # exact certificates settle 86 queries at step 4 already
    c["se3_a0"] = functools.partial(aligned_case, 12, N_MAIN, alpha=0.0, seed=12, w0=0.4, t0=0.1)
    c["se3_a3_rot"] = lambda: aligned_case(12, N_MAIN, alpha=3.0, seed=13, t0=0.0)
    c["se3_a3_trans"] = lambda: aligned_case(12, N_MAIN, alpha=3.0, seed=14, w0=0.0, t0=0.3)
    c["r3_x10"] = lambda: aligned_case(3, N_MAIN, seed=15, delta=0.2, scale=10.0)
    c["se3_a3_x10"] = lambda: aligned_case(12, N_MAIN, alpha=3.0, seed=16, delta=0.2, scale=10.0)
    c["r3_restart6"] = lambda: aligned_case(3, N_MAIN, seed=11, restart_at=6)
    return c


def size_cases():
    c = {}
    for dim in (3, 12):
        for nq in (1, 63, 64, 65):
            for nd in ("3nq", 1, 2):
                def make(dim=dim, nq=nq, nd=nd):
                    k = aligned_case(dim, nq, alpha=2.0, seed=100 + nq, steps=8)
                    if nd != "3nq":
                        k["data"] = np.ascontiguousarray(k["data"][:nd])
                    return k
                c["size_d%d_q%d_t%s" % (dim, nq, nd)] = make
    return c


def tie_case(dim, steps=10):
    """Exact ties: coordinates on a 2^-10 grid, frames signed permutations, alpha = 2, poses grid
    translations in y / z (exact in f64), the last 4 bitwise the identity; the two targets of a
    query differ from it by -/+ 2^-6 in x, so they tie exactly at every step."""
    rng = np.random.default_rng(7)
    g = np.arange(-2, 3) * 0.25
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.integers(-8, 9, (125, 3)) * 2.0 ** -10
    n = len(p)
    if dim == 12:
        perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2)]
        X = np.zeros((n, 3, 3))
        for i in range(n):
            pm = perms[rng.integers(6)]
            for c in range(3):
                X[i, pm[c], c] = rng.choice([-1.0, 1.0])
        M0 = np.concatenate([2.0 * X[:, :, c] for c in range(3)] + [p], axis=1)
    else:
        M0 = p
    off = np.zeros(dim)
    off[dim - 3] = 2.0 ** -6
    data = np.concatenate([M0 - off, M0 + off])[rng.permutation(2 * n)]
    poses = np.tile(np.eye(4), (steps, 1, 1))
    for k in range(steps - 4):
        poses[k, 1:3, 3] = rng.integers(-16, 17, 2) * 2.0 ** -9
    return dict(dim=dim, alpha=2.0, query=M0, data=np.ascontiguousarray(data), poses=poses, restart_at=0)


def ring_case(steps=300, n=130):
    """Ring age: the pose of step 1 is a move, steps 2 .. 257 are bitwise the identity (every
    query keeps its certificate of step 2, or of step 1, without a search), step 258 moves the
    queries along their lines far enough to flip designed ones -- when pose-ring row 2 has just
    been rewritten, so a certificate of step 2 must not be used."""
    k = aligned_case(3, n, seed=21, steps=2)
    g = np.random.default_rng(21)                 # the twist the generator drew (its first draws)
    w, t = _unit(g, 1, 3)[0] * 0.27, _unit(g, 1, 3)[0] * 0.07
    poses = np.tile(np.eye(4), (steps, 1, 1))
    poses[0] = exp_se3(w, t)
    move = 0.02 * 0.1 / 0.2                       # ~ delta / 10 along u_i (|xi M0| ~ 0.2)
    poses[257:] = exp_se3(-move * w, -move * t)
    k["poses"] = poses
    return k


# ------------------------------------------------------------------ long-double brute force
def _top(case, q64, qld, data, data_ld):
    """Per query: the candidates' indices sorted by (long-double distance, index) and those
    distances (nq, K).  An f64 pass shortlists; candidates beyond the K-th are farther than the
    second best by more than 1e-9 relative (asserted), far above f64 rounding."""
    nq, nd = len(q64), len(data)
    K = min(K_SHORT, nd)
    cand = np.empty((nq, K), np.int64)
    for a in range(0, nq, 128):
        d2 = ((q64[a:a + 128, None, :] - data[None, :, :]) ** 2).sum(-1)
        if K < nd:
            part = np.argpartition(d2, K - 1, axis=1)[:, :K]
            rest_min = np.partition(d2, K, axis=1)[:, K]
            second = np.sort(np.take_along_axis(d2, part, 1), axis=1)[:, min(1, K - 1)]
            assert (rest_min > second * (1.0 + 1e-9)).all(), "more than K_SHORT near-ties: raise K_SHORT"
        else:
            part = np.tile(np.arange(nd), (d2.shape[0], 1))
        cand[a:a + 128] = part
    dl = np.sqrt(((qld[:, None, :] - data_ld[cand]) ** 2).sum(-1))
    order = np.lexsort((cand, dl), axis=1)
    return np.take_along_axis(cand, order, 1), np.take_along_axis(dl, order, 1)


def _f32_mid_near(v):
    """For long-double values v: float32(v) and whether v is within 2^-45 relative of a float
    rounding midpoint (there an f64-evaluated distance may round to the neighbour)."""
    f = v.astype(np.float32)
    lo = (f.astype(LD) + np.nextafter(f, np.float32(-np.inf)).astype(LD)) / 2
    hi = (f.astype(LD) + np.nextafter(f, np.float32(np.inf)).astype(LD)) / 2
    gap = np.minimum(np.abs(v - lo), np.abs(hi - v))
    return f, (gap < v * LD(2.0) ** -45) & (v > 0)


def reference(case):
    """The brute force per step: a list of dicts with q (nq, dim) long double, best (nq), d1 and d2
    (long-double distances to the best and the nearest other target, inf without one), gap_ok (the
    best / runner-up gap in d^2 is 0 (an exact tie) or >= 1e3 roundings), anchor (long-double
    distance of the translation parts / points to the best's)."""
    dim, data = case["dim"], case["data"]
    data_ld = data.astype(LD)
    tn = np.sqrt((data ** 2).sum(1)).max()
    out, cache = [], {}
    for T in case["poses"]:
        key = T.tobytes()
        if key not in cache:
            qld = apply_pose(T, case["query"], dim)
            q64 = qld.astype(np.float64)
            cand, dl = _top(case, q64, qld, data, data_ld)
            best, d1 = cand[:, 0], dl[:, 0]
            d2 = dl[:, 1] if dl.shape[1] > 1 else np.full(len(d1), np.inf, LD)
            # roundings of the two squared distances as the engine's f64 arithmetic forms them:
            # 4 eps d^2 of the sums, and the query's own rounding (|dq| <= 6 eps |q|) times 2 d
            qn = np.sqrt((q64 ** 2).sum(1))
            rnd = EPS * (4.0 * (d2.astype(np.float64) ** 2) + 12.0 * d2.astype(np.float64) * (qn + tn))
            gap = (d2 ** 2 - d1 ** 2).astype(np.float64)
            gap_ok = (gap == 0.0) | (gap >= 1e3 * rnd) | ~np.isfinite(gap)
            a = slice(9, 12) if dim == 12 else slice(0, 3)
            anchor = np.sqrt(((qld[:, a] - data_ld[best][:, a]) ** 2).sum(1))
            cache[key] = dict(q=qld, best=best, d1=d1, d2=d2, gap_ok=gap_ok, tie=(gap == 0.0), anchor=anchor,
                              cand=cand, cand_d=dl)
        out.append(cache[key])
    return out


def phase_start(case, k):
    r = case["restart_at"]
    return r if (r > 0 and k >= r) else 1


def dist_ld(ref, k, ci):
    """|q_k - q_ci| in long double (steps 1-based)."""
    return np.sqrt(((ref[k - 1]["q"] - ref[ci - 1]["q"]) ** 2).sum(1))


def design_figures(case, ref):
    """Arg-min changes between consecutive steps: total and per step (index k - 1: step k against k - 1)."""
    ch = [0] + [int((ref[k]["best"] != ref[k - 1]["best"]).sum()) for k in range(1, len(ref))]
    return dict(changes=int(sum(ch)), per_step=ch, excused=int(sum((~r["gap_ok"]).sum() for r in ref)))


# ------------------------------------------------------------------ numpy models of the certificates
def ideal_model(case, ref, dl_factor=1.0, ring_leq=False):
    """Exact certificates: D1 = the exact distance to the match, L2 = to the nearest other target,
    dl = the exact displacement times dl_factor; the outputs of se3icp_nn_sequence (long-double
    certificate words).  ring_leq: the planted ring-age defect (a certificate of age kHist is used,
    against the pose that has overwritten its row: dl = 0)."""
    n, S = len(case["query"]), len(ref)
    out = {k: np.zeros((S, n), t) for k, t in (("idx", np.int32), ("dist", np.float32), ("cert_d1", LD),
                                               ("cert_l2", LD), ("cert_iter", np.int32), ("cert_j", np.int32))}
    out.update({k: np.zeros(S, np.int32) for k in ("searched", "single", "rechecked")})
    ci, j = np.full(n, -1), np.full(n, -1)
    D1, L2 = np.zeros(n, LD), np.zeros(n, LD)
    for k in range(1, S + 1):
        r, ps = ref[k - 1], phase_start(case, k)
        age_ok = (k - ci <= K_HIST) if ring_leq else (k - ci < K_HIST)
        usable = (ci >= ps) & (ci < k) & age_ok
        dl = np.zeros(n, LD)
        for c in np.unique(ci[usable]):
            m = usable & (ci == c)
            dl[m] = 0 if k - c == K_HIST else dist_ld(ref, k, int(c))[m] * LD(dl_factor)
        settle = usable & (D1 + dl < L2 - dl)
        s = ~settle
        tie = r["tie"]
        j[s], D1[s], L2[s] = r["best"][s], r["d1"][s], r["d2"][s]
        ci[s] = np.where(tie[s], -1, k)                    # an exact tie is re-resolved: no certificate
        out["idx"][k - 1], out["cert_iter"][k - 1], out["cert_j"][k - 1] = j, ci, np.where(ci < 0, 0, j)
        out["cert_d1"][k - 1], out["cert_l2"][k - 1] = np.where(ci < 0, 0, D1), np.where(ci < 0, 0, L2)
        a = slice(9, 12) if case["dim"] == 12 else slice(0, 3)
        out["dist"][k - 1] = np.sqrt(((r["q"][:, a] - case["data"].astype(LD)[j][:, a]) ** 2).sum(1)).astype(np.float32)
        out["searched"][k - 1], out["rechecked"][k - 1] = s.sum(), (s & tie).sum()
    return out


def f32_err(d, na, nb, D):
    """csrc/nn_cert.hpp f32_err in float32 arithmetic."""
    d, s = np.asarray(d, np.float32), np.float32(na) + np.float32(nb)
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        return f(1.25) * (f(2) * U32 * s * np.sqrt(np.maximum(d, f(0))) + f(D + 3) * U32 * d + f(4) * U32 * U32 * s * s) + f(1e-30)


def entry_norms(case, q64):
    """na (per query) and nb as se3icp_nn_sequence and the searches set them."""
    cen = case["data"].mean(0) if case["dim"] == 3 else np.zeros(case["dim"])
    nb = np.float32(np.sqrt(((case["data"] - cen) ** 2).sum(1)).max() * (1 + 1e-6))
    na = np.sqrt(((q64 - cen) ** 2).sum(1)).astype(np.float32) * np.float32(1.000001)
    return na, nb, cen


def header_model(case, ref, defect=None):
    """A restatement of csrc/nn_cert.hpp around an idealised search: f32 distances of the f32-rounded
    vectors, the widened radius, a target skipped when the f32 bound of its own inflated box
    (k_tree_leafbox) is >= thr -- except the match's three index neighbours, which stand for its
    leaf -- the flag, D1 / L2, the displacement bound and the settle predicate.  defect: None,
    "dl999" (dl x 0.999), "l2_d2_only" (L2 without the thr branch), "d1_no_err" (D1 without err)."""
    f = np.float32
    D, n, S = case["dim"], len(case["query"]), len(ref)
    a2 = case["alpha"] ** 2 if D == 12 else 0.0
    out = {k: np.zeros((S, n), t) for k, t in (("idx", np.int32), ("dist", np.float32), ("cert_d1", np.float32),
                                               ("cert_l2", np.float32), ("cert_iter", np.int32), ("cert_j", np.int32))}
    out.update({k: np.zeros(S, np.int32) for k in ("searched", "single", "rechecked")})
    data = case["data"]
    nd = len(data)
    q64s = [r["q"].astype(np.float64) for r in ref]
    _, nb, cen = entry_norms(case, q64s[0])
    tf = (data - cen).astype(f)
    # (the kernel's inflation is one fused multiply-add: tree_cases.inflation_fused, exact)
    infl = inflation_fused(tf)
    lo, hi = tf - infl, tf + infl
    ci, j = np.full(n, -1), np.full(n, -1)
    D1, L2 = np.zeros(n, f), np.zeros(n, f)
    tr = slice(9, 12) if D == 12 else slice(0, 3)
    qnorm = lambda q: np.sqrt(3.0 * a2 * (1.0 + 1e-12) + (q[:, tr] ** 2).sum(1))
    for k in range(1, S + 1):
        r, ps, T, q = ref[k - 1], phase_start(case, k), case["poses"][k - 1], q64s[k - 1]
        usable = (ci >= ps) & (ci < k) & (k - ci < K_HIST)
        settle = np.zeros(n, bool)
        for c in np.unique(ci[usable]):
            m = usable & (ci == c)
            Tr, qr = case["poses"][c - 1], q64s[c - 1]
            dt = np.sqrt(((q[:, tr] - qr[:, tr]) ** 2).sum(1))
            fro = ((T[:3, :3] - Tr[:3, :3]) ** 2).sum()
            dl = np.sqrt(a2 * fro * (1.0 + 1e-12) + dt * dt) * (1.0 + 1e-12) + 2e-15 * (qnorm(q) + qnorm(qr))
            if defect == "dl999":
                dl = dl * 0.999
            a, b = L2.astype(np.float64) - dl, D1.astype(np.float64) + dl
            M = 2.0 * qnorm(q) + b
            settle |= m & (a > b) & ((a - b) * (a + b) > 1e-14 * M * M)
        s = np.nonzero(~settle)[0]
        if len(s):
            na = entry_norms(case, q)[0][s]
            qf = (q[s] - cen).astype(f)
            mrg = np.zeros(len(s), f)
            if k >= 2 and (D == 3 or k - ps + 1 >= 4):
                mrg = np.sqrt(((q[s] - q64s[k - 2][s]) ** 2).sum(1)).astype(f)
            d1 = np.empty(len(s), f); d2 = np.empty(len(s), f); thr = np.empty(len(s), f); i1 = np.empty(len(s), np.int64)
            for c0 in range(0, len(s), 64):
                sl = slice(c0, c0 + 64)
                e = qf[sl, None, :] - tf[None, :, :]
                df = np.zeros(e.shape[:2], f)
                for x in range(D):
                    df = e[:, :, x] * e[:, :, x] + df
                b1 = df.argmin(1)
                rows = np.arange(len(b1))
                a1 = df[rows, b1]
                oth = df.copy(); oth[rows, b1] = np.inf
                a2nd = oth.min(1) if nd > 1 else np.full(len(b1), np.inf, f)
                ee = np.sqrt(a1) + f(2) * mrg[sl]
                t = np.maximum(a1, np.minimum(ee * ee, a2nd))
                th = t + f(3) * f32_err(t, na[sl], nb, D)
                eb = np.maximum(np.maximum(lo[None] - qf[sl, None, :], qf[sl, None, :] - hi[None]), f(0))
                lb = np.zeros(e.shape[:2], f)
                for x in range(D):
                    lb = eb[:, :, x] * eb[:, :, x] + lb
                visited = ~(lb * f(1 - 2e-6) >= th[:, None])
                visited |= (np.arange(nd)[None, :] // 4) == (b1[:, None] // 4)
                vo = np.where(visited, oth, np.inf)
                d1[sl], i1[sl], thr[sl] = a1, b1, th
                d2[sl] = vo.min(1) if nd > 1 else np.inf
            with np.errstate(invalid="ignore"):
                flag = ~(d2 - d1 > f(2) * f32_err(d2, na, nb, D))
            e1 = f32_err(d1, na, nb, D)
            if defect == "d1_no_err":
                e1 = f(0)
            with np.errstate(invalid="ignore"):
                l2sq = np.minimum(d2 - f32_err(d2, na, nb, D), thr * f(1 - 4e-6))
                if defect == "l2_d2_only":
                    l2sq = d2 - f32_err(d2, na, nb, D)
            nD1 = np.sqrt(d1 + e1) * f(1 + 1e-6)
            nL2 = np.sqrt(np.maximum(l2sq, f(0))) * f(1 - 1e-6)
            j[s] = np.where(flag, r["best"][s], i1)        # flagged: the exact f64 re-resolution
            ci[s] = np.where(flag, -1, k)
            D1[s], L2[s] = np.where(flag, f(0), nD1), np.where(flag, f(0), nL2)
            out["rechecked"][k - 1] = flag.sum() if nd > 1 else 0
        out["searched"][k - 1] = len(s)
        out["idx"][k - 1], out["cert_iter"][k - 1], out["cert_j"][k - 1] = j, ci, np.where(ci < 0, 0, j)
        out["cert_d1"][k - 1], out["cert_l2"][k - 1] = D1, L2
        out["dist"][k - 1] = np.sqrt(((r["q"][:, tr] - data.astype(LD)[j][:, tr]) ** 2).sum(1)).astype(f)
    return out


# ------------------------------------------------------------------ the checker
def check_run(case, ref, out):
    """The four checks of DESIGN section 23 on the outputs of se3icp_nn_sequence (or of a model)
    against the long-double brute force.  Returns violation counts (all zero for a sound run) and
    the recorded figures."""
    D, n, S = case["dim"], len(case["query"]), len(ref)
    nd = len(case["data"])
    data_ld = case["data"].astype(LD)
    tr = slice(9, 12) if D == 12 else slice(0, 3)
    v = dict(idx=0, dist=0, cert_j=0, d1=0, l2=0, tight=0, settle_match=0, settle_ineq=0, settle_age=0,
             nocert=0, counters=0)
    fig = dict(steps=S, queries=n, settled=0, ulp1=0, searched=int(out["searched"].sum()),
               single=int(out["single"].sum()), rechecked=int(out["rechecked"].sum()),
               max_d1_slack=0.0, min_l2_slack=float("inf"), settled_per_step=[])
    words = [out[k] for k in ("cert_d1", "cert_l2", "cert_iter", "cert_j")]
    for k in range(1, S + 1):
        r, ps = ref[k - 1], phase_start(case, k)
        idx, ci = out["idx"][k - 1].astype(np.int64), out["cert_iter"][k - 1]
        d1w, l2w = out["cert_d1"][k - 1].astype(LD), out["cert_l2"][k - 1].astype(LD)
        # 1. result
        wrong = idx != r["best"]
        v["idx"] += int(wrong.sum())
        want, near = _f32_mid_near(r["anchor"])
        got = out["dist"][k - 1]
        ok = ~wrong
        exact = got.view(np.uint32) == want.view(np.uint32)
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1
        v["dist"] += int((ok & ~np.where(near, ulp, exact)).sum())
        fig["ulp1"] += int((ok & near & ~exact & ulp).sum())
        # 2. search certificate
        m = ci == k
        v["cert_j"] += int((m & (out["cert_j"][k - 1] != idx)).sum())
        # (distances to the CERTIFIED match and to every other target, from the candidates)
        cj = out["cert_j"][k - 1].astype(np.int64)
        dj = np.sqrt(((r["q"] - data_ld[cj]) ** 2).sum(1))
        oth = np.where(r["cand"][:, 0] == cj, r["d2"], r["d1"])
        v["d1"] += int((m & ~(dj <= d1w)).sum())
        v["l2"] += int((m & ~(oth >= l2w)).sum())
        if m.any():
            na, nb, _ = entry_norms(case, r["q"].astype(np.float64))
            dj2 = (dj ** 2).astype(np.float64)
            bar = (dj2 + 2.1 * f32_err(dj2, na, nb, D).astype(np.float64)) * (1 + 3e-6)
            if out["cert_d1"].dtype == np.float32:          # (the tightness bar is the header's: f32 certificates)
                v["tight"] += int((m & ~((d1w ** 2).astype(np.float64) <= bar)).sum())
            pos = m & (dj > 0)
            if pos.any():
                fig["max_d1_slack"] = max(fig["max_d1_slack"], float((d1w[pos] / dj[pos] - 1).max()))
            fin = m & np.isfinite(oth.astype(np.float64))
            if fin.any():
                fig["min_l2_slack"] = min(fig["min_l2_slack"], float((1 - l2w[fin] / oth[fin]).min()))
        # 3. settle
        st = (ci >= 0) & (ci < k)
        fig["settled"] += int(st.sum())
        fig["settled_per_step"].append(int(st.sum()))
        for c in np.unique(ci[st]):
            mm = st & (ci == c)
            same = np.ones(n, bool)
            for w in words:
                same &= w[k - 1] == w[c - 1]
            v["counters"] += int((mm & ~same).sum())      # a settled query's words are those of step ci
            mm &= same
            v["settle_match"] += int((mm & (idx != cj)).sum())
            dl = dist_ld(ref, k, int(c))
            v["settle_ineq"] += int((mm & ~(d1w + dl < l2w - dl)).sum())
            if not (c >= ps and k - c < K_HIST):
                v["settle_age"] += int(mm.sum())
        # 4. no certificate / counters
        no = ci == -1
        if nd > 1:
            v["nocert"] += int(no.sum() != out["rechecked"][k - 1])
        v["counters"] += int(out["searched"][k - 1] != (m | no).sum())
        if k > 1:
            prev_no = out["cert_iter"][k - 2] == -1
            v["nocert"] += int((prev_no & st).sum())        # searched again at the next step
    return v, fig


def ideal_settles(case, ref):
    out = ideal_model(case, ref)
    _, fig = check_run(case, ref, out)
    return fig["settled"], fig["settled_per_step"]
