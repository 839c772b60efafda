"""The setup stage's per-point arithmetic restated in numpy.longdouble (64-bit mantissa on
x86-64), vectorised over points, from the reference's formulas:

    kNN       KDTreeFlann::SearchKNN of every point in its own cloud (ISR.cpp:253): brute force,
              ordered by (d^2, index), the point itself at rank 0
    TOLDI     computeSingleTOLDISE3Frame (ISR.cpp:241-316), with kk = min(k, n), rz = kk // 3:
                c     = sum over ranks 1 .. rz-1 of p, divided by rz     (the quirk centroid)
                C     = sum over ranks 1 .. rz of (p - c)(p - c)^T
                z*    = eigenvector of C's smallest eigenvalue, with z* . sum_{1..kk-1} v >= 0,
                        v = p - q
                R     = |v| at rank kk - 1
                w_i   = (R - |v_i|)^2 (z . v_i)^2
                x_raw = sum w_i v_i - ((sum w_i v_i) . z) z,  x = x_raw / |x_raw|,  y = z x x
    normals   Open3D EstimateNormals (ISR.cpp:643): the centred covariance of ranks 0 .. kn-1,
              kn = min(k, n), its smallest eigenvector; (0, 0, 1) when kn < 3

Eigenvectors: cyclic Jacobi in long double, 12 sweeps (test_lrf_reference.py holds it against
mpmath at 40 digits).  The x axis takes the z to use as an argument, so it can be evaluated at
the z under test: then the x measure sees rounding only, not the conditioning of z.

The measures (eps = 2^-52; everything but the value under test comes from this module, the gap
is lambda_1 - lambda_0 of this module's matrix):

    K_z = |z - z*| gap / (eps sum_{ranks 1..rz} |p - c|^2)
    K_x = |x - x*(z under test)| |x_raw| / (eps sum w_i |v_i|)
    K_n = min(|n - n*|, |n + n*|) gap / (eps mean_{ranks} |p|^2)

Each is the error in units of the first-order rounding error of the quantity's own sums: an
eigenvector moves by |dC| / gap when its matrix moves by dC, and a sum of f64 products is off by
eps times the sum of the magnitudes.  The normal's scale is the raw second moment because the
reference forms cumulants of raw coordinates, so a cloud far from the origin loses digits there
by design.  An implementation that rounds like f64 stays at order one on all three whatever the
conditioning; a wrong rank range, divisor, radius or weight is off by many orders (DEFECTS, the
power test in test_lrf_reference.py).

The designed clouds (cloud()) and their k lists (CASES) are chosen so that no point needs leaving
out: test_lrf_reference.py asserts the gaps, the x-axis ratios and the z-sign margins.
"""
import functools

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
BAR_FACTOR = 8  # the engine's bars (test_gpu_frames.py) are this many times the oracle's maxima

# planted defects of the restatement (the power test): name -> what it changes
DEFECTS = ("cov_ranks",      # covariance over ranks 1 .. rz-1
           "centroid_div",   # centroid divided by rz - 1
           "radius_rank",    # R taken from rank kk - 2
           "weight_unsq",    # the (z . v) weight unsquared
           "no_self")        # normals without the self point

K_512 = (9, 10, 11, 12, 23, 24, 25, 26, 27, 30, 48, 51, 64, 65, 90, 127, 128, 129, 150)
K_FEW = (30, 90)
CASES = {"surface": K_512, "slab": K_512, "ball": K_512, "offset": K_512,
         "surface517": K_FEW, "surface4099": K_FEW, "small20": K_FEW, "small7": K_FEW}
K_MAX = 150
SEEDS = {"surface": 11, "slab": 12, "ball": 13, "offset": 14, "surface517": 15, "surface4099": 16, "small20": 17,
         "small7": 18}


def _surface(rng, n):
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    z = 0.3 * xy[:, 0] ** 2 - 0.2 * xy[:, 1] ** 2 + 0.02 * rng.standard_normal(n)
    return np.column_stack([xy, z])


@functools.lru_cache(maxsize=None)
def cloud(kind):
    """The designed cloud `kind` as (n, 3) f64 (read-only)."""
    rng = np.random.default_rng(SEEDS[kind])
    if kind == "surface":
        p = _surface(rng, 512)
    elif kind == "slab":
        p = np.column_stack([rng.uniform(-1.0, 1.0, (512, 2)), 1e-3 * rng.standard_normal(512)])
    elif kind == "ball":
        p = rng.standard_normal((512, 3))
    elif kind == "offset":
        p = _surface(rng, 512) + np.array([100.0, -200.0, 50.0])
    elif kind == "surface517":
        p = _surface(rng, 517)
    elif kind == "surface4099":
        p = _surface(rng, 4099)
    elif kind == "small20":
        p = _surface(rng, 20)
    elif kind == "small7":
        p = _surface(rng, 7)
    else:
        raise KeyError(kind)
    p = np.ascontiguousarray(p, dtype=np.float64)
    p.setflags(write=False)
    return p


def plane_cloud():
    """An exact plane: xy as in `slab`, z = 0.25."""
    rng = np.random.default_rng(SEEDS["slab"])
    return np.ascontiguousarray(np.column_stack([rng.uniform(-1.0, 1.0, (512, 2)), np.full(512, 0.25)]))


# ------------------------------------------------------------------------------------ kNN
def knn_ld(pts, k, chunk=128):
    """The min(k, n) nearest of every point in its own cloud, by (d^2, index) with d^2 in long
    double: (n, min(k, n)) int32.  The point itself has d^2 = 0 and comes first (or, among
    exact duplicates, the lowest index does)."""
    P = np.asarray(pts, dtype=np.float64).astype(LD)
    n = P.shape[0]
    kk = min(k, n)
    out = np.empty((n, kk), np.int32)
    for lo in range(0, n, chunk):
        d = P[lo:lo + chunk, None, :] - P[None, :, :]
        d2 = (d * d).sum(2)
        if n > 4 * kk:  # the kk smallest first, then those in order (ties keep index order)
            kth = np.partition(d2, kk - 1, axis=1)[:, kk - 1]
            for r in range(d2.shape[0]):
                cand = np.nonzero(d2[r] <= kth[r])[0]
                out[lo + r] = cand[np.argsort(d2[r, cand], kind="stable")][:kk]
        else:
            out[lo:lo + chunk] = np.argsort(d2, axis=1, kind="stable")[:, :kk]
    return out


@functools.lru_cache(maxsize=None)
def knn_of(kind):
    """knn_ld of the designed cloud at K_MAX; the list for a smaller k is its prefix."""
    idx = knn_ld(cloud(kind), K_MAX)
    idx.setflags(write=False)
    return idx


def padded(idx, k):
    """The first k columns of idx, filled with -1 past its width (what the entries return for k > n)."""
    n, w = idx.shape
    out = np.full((n, k), -1, np.int32)
    out[:, :min(k, w)] = idx[:, :k]
    return out


# ------------------------------------------------------------------------------------ eigen
def jacobi_eigh_ld(C, sweeps=12):
    """Eigenvalues (ascending) and eigenvectors (columns) of symmetric (m, 3, 3) matrices by
    cyclic Jacobi rotations in long double."""
    a = np.array(C, dtype=LD)
    a = (a + a.transpose(0, 2, 1)) / 2
    m = a.shape[0]
    v = np.broadcast_to(np.eye(3, dtype=LD), (m, 3, 3)).copy()
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = a[:, p, q]
            nz = apq != 0
            with np.errstate(over="ignore"):  # (a vanishing a_pq: tau overflows and t becomes 0)
                tau = (a[:, q, q] - a[:, p, p]) / (2 * np.where(nz, apq, LD(1)))
                t = np.where(nz, np.where(tau >= 0, LD(1), LD(-1)) / (np.abs(tau) + np.sqrt(tau * tau + 1)), LD(0))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            # a <- G^T a G, v <- v G with the rotation G = [[c, s], [-s, c]] in the (p, q) plane
            c, s = c[:, None], s[:, None]
            a[:, :, p], a[:, :, q] = c * a[:, :, p] - s * a[:, :, q], s * a[:, :, p] + c * a[:, :, q]
            a[:, p, :], a[:, q, :] = c * a[:, p, :] - s * a[:, q, :], s * a[:, p, :] + c * a[:, q, :]
            a[:, p, q] = a[:, q, p] = 0
            v[:, :, p], v[:, :, q] = c * v[:, :, p] - s * v[:, :, q], s * v[:, :, p] + c * v[:, :, q]
    w = np.stack([a[:, 0, 0], a[:, 1, 1], a[:, 2, 2]], 1)
    order = np.argsort(w, axis=1, kind="stable")
    w = np.take_along_axis(w, order, 1)
    v = np.take_along_axis(v, order[:, None, :], 2)
    return w, v


def _norm(a):
    return np.sqrt((a * a).sum(-1))


# ------------------------------------------------------------------------------------ TOLDI
def toldi_z(pts, idx, k, defects=()):
    """Everything of the frame up to the oriented z axis, for every point: a dict with
    z (n, 3), lam (n, 3) ascending, gap, scale_z = sum_{1..rz} |p - c|^2, sv = sum v,
    sabs_v = sum |v|, and the parts the x axis needs (v, vn, R)."""
    P = np.asarray(pts, dtype=np.float64).astype(LD)
    n = P.shape[0]
    kk = min(k, n)
    rz = kk // 3
    nb = P[idx[:, :kk]]
    c = nb[:, 1:rz].sum(1) / LD(rz - 1 if "centroid_div" in defects else rz)
    d = nb[:, 1:(rz if "cov_ranks" in defects else rz + 1)] - c[:, None, :]
    C = np.einsum("nki,nkj->nij", d, d)
    lam, V = jacobi_eigh_ld(C)
    z = V[:, :, 0]
    v = nb[:, 1:] - P[:, None, :]
    sv = v.sum(1)
    z = np.where(((z * sv).sum(1) < 0)[:, None], -z, z)
    vn = _norm(v)
    R = vn[:, kk - 3] if "radius_rank" in defects else vn[:, kk - 2]  # v starts at rank 1
    return {"z": z, "lam": lam, "gap": lam[:, 1] - lam[:, 0], "scale_z": (d * d).sum((1, 2)), "C": C,
            "sv": sv, "sabs_v": vn.sum(1), "v": v, "vn": vn, "R": R, "defects": tuple(defects)}


def toldi_x(parts, z):
    """The x axis at the given z (n, 3): (x, |x_raw|, sum |w_i| |v_i|)."""
    z = np.asarray(z).astype(LD)
    v, vn, R = parts["v"], parts["vn"], parts["R"]
    zv = np.einsum("nki,ni->nk", v, z)
    w = (R[:, None] - vn) ** 2 * (zv if "weight_unsq" in parts["defects"] else zv * zv)
    a = np.einsum("nk,nki->ni", w, v)
    x_raw = a - (a * z).sum(1)[:, None] * z
    xr = _norm(x_raw)
    return x_raw / xr[:, None], xr, (np.abs(w) * vn).sum(1)


def normals_ld(pts, idx, k, defects=()):
    """(n* (n, 3), gap, mean |p|^2 over the ranks used, lam) of every point."""
    P = np.asarray(pts, dtype=np.float64).astype(LD)
    n = P.shape[0]
    kn = min(k, n)
    if kn < 3:
        e3 = np.broadcast_to(np.array([0, 0, 1], LD), (n, 3)).copy()
        return e3, np.full(n, np.inf, LD), np.ones(n, LD), np.zeros((n, 3), LD)
    nb = P[idx[:, (1 if "no_self" in defects else 0):kn]]
    d = nb - nb.mean(1)[:, None, :]
    C = np.einsum("nki,nkj->nij", d, d) / LD(nb.shape[1])
    lam, V = jacobi_eigh_ld(C)
    return V[:, :, 0], lam[:, 1] - lam[:, 0], (nb * nb).sum((1, 2)) / LD(nb.shape[1]), lam


# ------------------------------------------------------------------------------------ measures
def frame_measures(parts, frames):
    """The conditioned measures of (n, 4, 4) f64 frames against `parts` (toldi_z's dict):
    K_z, K_x per point, |y - z x x|_inf per point, and z . sum v per point."""
    F = np.asarray(frames, dtype=np.float64)
    x, y, z = (F[:, :3, j].astype(LD) for j in range(3))
    kz = _norm(z - parts["z"]) * parts["gap"] / (EPS * parts["scale_z"])
    xs, xr, sw = toldi_x(parts, F[:, :3, 2])
    kx = _norm(x - xs) * xr / (EPS * sw)
    ydev = np.abs(y - np.cross(z, x)).max(1)
    return kz.astype(np.float64), kx.astype(np.float64), ydev.astype(np.float64), (z * parts["sv"]).sum(1)


def normal_measure(ref, normals):
    """K_n per point of (n, 3) f64 normals against ref = normals_ld(...)."""
    ns, gap, scale, _ = ref
    g = np.asarray(normals, dtype=np.float64).astype(LD)
    return (np.minimum(_norm(g - ns), _norm(g + ns)) * gap / (EPS * scale)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(kind, k):
    """(toldi_z parts, normals_ld tuple) of the designed cloud `kind` at k, computed once."""
    pts, idx = cloud(kind), knn_of(kind)
    return toldi_z(pts, idx, k), normals_ld(pts, idx, k)


@functools.lru_cache(maxsize=None)
def oracle_measures():
    """The oracle (oracle/refcpu.cpp) measured against this module on every (kind, k) of CASES:
    {(kind, k): {"kz", "kx", "kn": per-point arrays, "frames", "normals": the oracle's output}}."""
    from oracle import refcpu
    out = {}
    for kind, ks in CASES.items():
        pts = cloud(kind)
        for k in ks:
            parts, nref = case(kind, k)
            fr, nr = refcpu.toldi_frames(pts, k), refcpu.estimate_normals(pts, k)
            kz, kx, ydev, zs = frame_measures(parts, fr)
            out[(kind, k)] = {"kz": kz, "kx": kx, "ydev": ydev, "zsv": zs, "kn": normal_measure(nref, nr),
                              "frames": fr, "normals": nr}
    return out


def oracle_maxima(kind=None):
    """(KZ_ORACLE, KX_ORACLE, KN_ORACLE): the oracle's largest K_z, K_x, K_n over every case (or
    over the k list of one kind)."""
    m = [v for (kd, _), v in oracle_measures().items() if kind is None or kd == kind]
    return tuple(float(max(np.max(v[key]) for v in m)) for key in ("kz", "kx", "kn"))
