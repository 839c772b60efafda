"""Inputs, long-double references and bars of the setup-record tests (test_gpu_setup_record.py on
the GPU, test_setup_record_host.py for the oracle alone on the same inputs).

The bars are derived, none is measured (u = 2^-53, half an ulp):

  centre, exact inputs   every coordinate a multiple of 2^-10 below 4 and at most 2^17 + 1 points:
                         a sum of them stays below 2^20 on a grid of 2^-10, 30 bits, so it is exact
                         in f64 in ANY order and the centre is one division: fsum / n, bit for bit.
  centre, generic        |c - c_ld| <= 1.01 (n - 1) u sum|x_i| / n + u |c| per axis: the classical
                         bound of a recursive sum in any order ((n - 1) u sum|x_i| to first order;
                         1.01 covers the higher orders for n u << 1) divided by n, plus the division.
  scale                  |s - s_ld| <= 8 u s_ld, s_ld = scale_pre (1 / rmax) with rmax in long double
                         about the RECORDED centres.  Every step of sqrt(dx^2 + dy^2 + dz^2) ->
                         1 / r -> scale_pre * (.) is at most half an ulp with or without contraction:
                         three products, two additions, a root, a reciprocal and a product.  With the
                         differences p - c (half an ulp each, they enter r^2 twice, the root halves
                         them): (2 + 1 + 2) / 2 + 1 + 1 + 1 = 5.5 u <= 8 u to first order.
  coordinates            (p + (-c)) * s from the recorded c and s: an addition, then a product;
                         nothing can contract, so numpy's f64 gives the same bits.
  confidence             |conf - conf_ld| <= 4 u (|p1| z^2 + |p2| z + |p3|) / |error(z)| |conf_ld|:
                         the first-order rounding of the polynomial's three terms in units of its own
                         conditioning (the constants are the f64 constants on both sides).
"""
import functools
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
GRID = 2.0 ** -10
K_CHUNK = 2048                       # kChunk (csrc/view.hpp)
EDGE_SIZES = (2047, 2048, 2049, 4097, 6145)
WRAP_SIZE = 64 * K_CHUNK + 1         # 65 chunks: lane 0 of k_pair_centers folds chunks 0 and 64
SCALE_BAR = 8 * U
FAR = np.array([3.5, -3.25, 3.0])    # on the grid; about 4.5 from every cloud centre below
UTM = np.array([4.5e5, 5.4e6, 120.0])


def _frozen(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def grid_cloud(n, seed, far=False):
    """n points on the 2^-10 grid inside a ball of radius 1.25 about a centre that depends on the
    seed (so two clouds of a pair have centres about 0.5 apart: a radius about the wrong centre
    misses); far: the LAST point, the last of the last chunk, is FAR, the pair's farthest."""
    rng = np.random.default_rng(7000 + seed)
    d = rng.normal(size=(n, 3))
    d *= (1.25 * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0) / np.linalg.norm(d, axis=1))[:, None]
    c = np.array([0.75, -0.5, 0.25]) + 0.3 * rng.uniform(-1.0, 1.0, 3)
    p = np.round((d + c) / GRID) * GRID
    if far:
        p[-1] = FAR
    assert np.array_equal(np.round(p / GRID) * GRID, p) and np.abs(p).max() < 4.0
    return _frozen(p)


def edge_pairs():
    """Four pairs over EDGE_SIZES; the farthest point of pairs 0 and 2 is the last point of the
    target's last (partial, or one-point) chunk, of pairs 1 and 3 the last point of the source's."""
    g = grid_cloud
    return [(g(2047, 1), g(2049, 2, True)), (g(4097, 3, True), g(2048, 4)),
            (g(2048, 5), g(6145, 6, True)), (g(6145, 7, True), g(4097, 8))]


def wrap_pairs():
    """More than 64 chunks on either side of a pair, the farthest point last."""
    g = grid_cloud
    return [(g(2049, 9), g(WRAP_SIZE, 10, True)), (g(WRAP_SIZE, 11, True), g(2048, 12))]


@functools.lru_cache(maxsize=None)
def utm_cloud(n, seed):
    """Generic coordinates at UTM-sized offsets."""
    rng = np.random.default_rng(7100 + seed)
    return _frozen(rng.normal(size=(n, 3)) * np.array([30.0, 25.0, 3.0]) + UTM + rng.uniform(-5.0, 5.0, 3))


def utm_pairs():
    return [(utm_cloud(6145, 1), utm_cloud(4097, 2)), (utm_cloud(2049, 3), utm_cloud(12289, 4)),
            (utm_cloud(517, 5), utm_cloud(2047, 6))]


@functools.lru_cache(maxsize=None)
def depth_cloud(n, seed):
    """Camera-frame points with depths over [0.4, 4], both ends included exactly."""
    rng = np.random.default_rng(7200 + seed)
    z = rng.uniform(0.4, 4.0, n)
    z[0], z[-1], z[n // 2] = 0.4, 4.0, 0.4
    xy = rng.uniform(-0.6, 0.6, (n, 2)) * z[:, None]
    return _frozen(np.column_stack([xy, z]))


def depth_pairs():
    return [(depth_cloud(2049, 1), depth_cloud(4097, 2)), (depth_cloud(517, 3), depth_cloud(2048, 4)),
            (depth_cloud(4097, 5), depth_cloud(2047, 6))]


# ------------------------------------------------------------------ references and bars
def center_exact(p):
    """fsum / n per axis: THE centre of a grid cloud (its sum is exact, see the module docstring)."""
    n = p.shape[0]
    return np.array([math.fsum(p[:, a].tolist()) / n for a in range(3)])


def center_ld(p):
    return (p.astype(LD).sum(0) / LD(p.shape[0]))


def center_sequential(p):
    """The oracle's get_center (oracle/refcpu.cpp: std::accumulate order, then / n) in f64."""
    return np.cumsum(p, axis=0)[-1] / p.shape[0]


def center_bound(p, c):
    n = p.shape[0]
    return 1.01 * (n - 1) * U * np.abs(p).sum(0) / n + U * np.abs(c)


def radii_ld(p, c):
    d = p.astype(LD) - np.asarray(c, dtype=np.float64).astype(LD)
    return np.sqrt((d * d).sum(1))


def scale_ld(src, tgt, cs, ct, scale_pre):
    """scale_pre * (1 / max(r_src, r_tgt)) in long double, each radius about its own cloud's centre
    (ISR.cpp:571-574); also (which side holds the farthest point, its index, the runner-up radius
    over rmax)."""
    rs, rt = radii_ld(src, cs), radii_ld(tgt, ct)
    side = int(rt.max() > rs.max())
    r = rt if side else rs
    rmax = r.max()
    rest = np.concatenate([np.delete(r, r.argmax()), rs if side else rt])
    return LD(scale_pre) * (LD(1) / rmax), (side, int(r.argmax()), float(rest.max() / rmax))


def scale_f64(src, tgt, cs, ct, scale_pre):
    """The same in f64, as the oracle computes it (oracle/refcpu.cpp, no contraction)."""
    def rad(p, c):
        d = p - c
        return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]).max()
    return scale_pre * (1.0 / max(rad(src, cs), rad(tgt, ct)))


def scale_deviation(s, s_ld):
    """|s - s_ld| / s_ld in units of SCALE_BAR."""
    return float(abs(LD(s) - s_ld) / s_ld / SCALE_BAR)


def normalized(p, c, s):
    """(p + (-c)) * s, one rounded operation per ufunc."""
    return np.ascontiguousarray((p + (-np.asarray(c, dtype=np.float64))) * np.float64(s))


P1, P2, P3, MIN_DEPTH = 0.002203, -0.001028, 0.0005351, 0.4


def conf_ld(z):
    z = np.asarray(z, dtype=np.float64).astype(LD)
    err = LD(P1) * z * z + LD(P2) * z + LD(P3)
    return (LD(P1) * LD(MIN_DEPTH) + LD(P2) * LD(MIN_DEPTH) + LD(P3)) / err


def conf_deviation(conf, z):
    """The relative error of conf per point in units of its bar."""
    z64 = np.asarray(z, dtype=np.float64)
    zl = z64.astype(LD)
    ref = conf_ld(z64)
    err = LD(P1) * zl * zl + LD(P2) * zl + LD(P3)
    bar = 4 * U * (abs(P1) * zl * zl + abs(P2) * zl + abs(P3)) / np.abs(err)
    return (np.abs(np.asarray(conf, dtype=np.float64).astype(LD) - ref) / np.abs(ref) / bar).astype(np.float64)


def frames_of_rows(rows):
    """(n, 4, 4) frames of (n, 12) unweighted rows (R00 R10 R20 R01 R11 R21 R02 R12 R22 t0 t1 t2)."""
    rows = np.asarray(rows, dtype=np.float64)
    F = np.zeros((rows.shape[0], 4, 4))
    for c in range(3):
        F[:, :3, c] = rows[:, 3 * c:3 * c + 3]
    F[:, :3, 3] = rows[:, 9:12]
    F[:, 3, 3] = 1.0
    return F


# ------------------------------------------------------------------ the designed clouds in a pair
FRAME_KINDS = ("surface517", "surface4099")
FRAME_KS = (90, 150)   # on each side of 128, where k_knn_big takes over


def designed_pair_normalization(scale_pre=3.0):
    """(centre, scale) of the pair (surface517, surface4099) in plain f64, for the CPU tie check."""
    import lrf_reference as L
    a, b = (L.cloud(k) for k in FRAME_KINDS)
    ca, cb = center_sequential(a), center_sequential(b)
    return (ca, cb), scale_f64(a, b, ca, cb, scale_pre)


# ------------------------------------------------------------------ tie inputs (test_gpu_lrf_take.py's)
def lattice(n, h):
    g = np.arange(n, dtype=np.float64) * h
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3))


def _symmetric_cluster(rng, centre, extra):
    v = rng.normal(size=(100, 3)) * np.linspace(0.05, 1.0, 100)[:, None]
    pts = [centre[None, :], centre + v, centre - v]
    if extra:
        pts.append(centre + 0.01 * rng.normal(size=(extra, 3)))
    return np.concatenate(pts)


def rounding_gap_clouds():
    """test_gap_at_rounding_level's clouds: two point-symmetric clusters, cloud 1 under two scales."""
    rng = np.random.default_rng(11)
    a = np.concatenate([_symmetric_cluster(rng, np.array([0.0, 0.0, 0.0]), 0),
                        _symmetric_cluster(rng, np.array([40.0, 3.0, -2.0]), 1),
                        rng.normal(size=(600, 3)) * 3.0 + np.array([20.0, 0.0, 0.0])])
    a = np.ascontiguousarray(a[rng.permutation(a.shape[0])])
    return [np.ascontiguousarray(a * 1.7 + 0.5), a, np.ascontiguousarray(a[:900] * 0.6)]
