"""GPU tests of the voxel-grid downsample (se3icp_voxel_downsample, _device; k_voxel.hip).

The bar is a numpy restatement in this file and no tolerance: `restate` computes the cells as
floor((p - (min - 0.5 v)) / v), one IEEE subtraction and one IEEE division, orders the voxels by
the lowest input index they hold and sums every voxel's points in input order by an explicit
loop over the rank within the voxel (the j-th point of every voxel is added in step j, from
+0.0), then divides by the count.  Every comparison is array_equal on the bytes of the points,
the counts and the first indices.

The engine takes one of three paths per voxel by its point count (voxel.hpp): up to 32 points
one lane, up to 2,048 a block ranking the members in LDS, beyond that a block compacting the
cloud; the clouds below put counts on both sides of both thresholds, and the sizes put point
counts on both sides of a wavefront, a block and the 1,024-point chunk.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mod():
    import se3icp
    se3icp.load()
    if se3icp.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on an MI355X")
    return se3icp


def restate(xyz, v, reciprocal=False):
    """(points, counts, first indices) of the downsample, see the module docstring.
    reciprocal: the cells by p * (1 / v) instead -- the form the engine must NOT compute."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float64)
    v = np.float64(v)
    mb = xyz.min(axis=0) - np.float64(0.5) * v
    d = xyz - mb
    q = d * (np.float64(1.0) / v) if reciprocal else d / v
    cell = np.floor(q).astype(np.int64)
    _, first, inv, counts = np.unique(cell, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first, kind="stable")          # voxels by first occurrence
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(order.size)
    vox = rank[inv]                                   # output voxel of every point
    perm = np.argsort(vox, kind="stable")             # points by voxel, input order within one
    cnt = counts[order].astype(np.int64)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    sums = np.zeros((cnt.size, 3))
    for j in range(int(cnt.max())):
        sel = np.nonzero(cnt > j)[0]
        sums[sel] = sums[sel] + xyz[perm[start[sel] + j]]
    out = sums / cnt.astype(np.float64)[:, None]
    return out, cnt.astype(np.int32), first[order].astype(np.int32)


def cells(xyz, v, reciprocal=False):
    mb = xyz.min(axis=0) - np.float64(0.5) * np.float64(v)
    d = xyz - mb
    return np.floor(d * (np.float64(1.0) / np.float64(v)) if reciprocal else d / np.float64(v)).astype(np.int64)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_host(mod, xyz, v, device=0, want=None):
    """The host entry against the restatement; returns the engine's (points, counts, firsts)."""
    want = want or restate(xyz, v)
    got = mod.voxel_downsample(xyz, v, device=device, return_counts=True)
    assert got[0].shape == want[0].shape, (got[0].shape, want[0].shape)
    assert np.array_equal(got[2], want[2]) and same(got[2], want[2])
    assert np.array_equal(got[1], want[1]) and same(got[1], want[1])
    bad = np.nonzero((got[0].view(np.uint64) != want[0].view(np.uint64)).any(axis=1))[0]
    assert same(got[0], want[0]), (bad.size, bad[:5], got[0][bad[:3]], want[0][bad[:3]], want[1][bad[:5]])
    only = mod.voxel_downsample(xyz, v, device=device)
    assert same(only, want[0])
    return got


# ------------------------------------------------------------------ inputs
def cube(n, seed):
    return np.random.default_rng(seed).random((n, 3))


EDGE_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097]


def division_cloud(axis, v):
    """0.5 v, then fl(k v) for k = 1 .. 4096 along `axis` (min_bound is exactly 0)."""
    k = np.arange(1, 4097, dtype=np.float64)
    line = np.concatenate([[np.float64(0.5) * np.float64(v)], k * np.float64(v)])
    xyz = np.zeros((line.size, 3))
    xyz[:, axis] = line
    return xyz


def tie_cloud():
    """Multiples of 0.125 in [-8, 8]: every quotient at voxel 0.25 is an integer or a half-integer.
    One point and its neighbours across a cell boundary are repeated."""
    rng = np.random.default_rng(11)
    xyz = rng.integers(-64, 65, size=(3000, 3)).astype(np.float64) * 0.125
    xyz[0] = (-8.0, -8.0, -8.0)  # pins min_bound to -8.125
    dup = np.array([[-0.125, 0.0, 0.125], [-0.125 + 0.125, 0.0, 0.125], [-0.125 - 0.125, 0.0, 0.125]])
    xyz = np.concatenate([xyz, np.repeat(dup, 5, axis=0), xyz[100:140]])
    return xyz[rng.permutation(xyz.shape[0])]


def utm_cloud():
    rng = np.random.default_rng(12)
    return np.array([5.1e5, 5.4e6, 300.0]) + rng.uniform(-40.0, 40.0, size=(20000, 3))


def sparse_cloud():
    """2,048 cells with indices from {0, 2^20 - 1} and random 20-bit values, 4 points each at
    shuffled positions: three 20-bit axes, a 60-bit key."""
    rng = np.random.default_rng(13)
    idx = rng.integers(0, 1 << 20, size=(2048, 3))
    ext = rng.integers(0, 8, size=(2048, 3))  # 0: the lowest cell, 1: the highest, else a random one
    idx = np.where(ext == 0, 0, np.where(ext == 1, (1 << 20) - 1, idx))
    idx[0] = 0
    idx[1] = (1 << 20) - 1
    pts = np.repeat(idx, 4, axis=0).astype(np.float64) + rng.uniform(0.5, 0.999, size=(8192, 3))
    pts[0] = 0.5  # min_bound = 0: the cell of a point is the integer part
    return pts[np.concatenate([[0], 1 + rng.permutation(8191)])]


def count_cloud(counts, seed):
    """A cloud whose voxels (voxel 1, cells along x) hold `counts` points, the first one more,
    interleaved."""
    rng = np.random.default_rng(seed)
    cell = np.repeat(np.arange(len(counts)), counts)
    pts = rng.uniform(0.5, 0.999, size=(cell.size, 3))
    pts[:, 0] += cell
    pts = pts[rng.permutation(cell.size)]
    return np.concatenate([[[0.5, 0.5, 0.5]], pts])  # min_bound = 0; cell 0 gets this point too


# ------------------------------------------------------------------ one cloud
@pytest.mark.parametrize("n", EDGE_SIZES)
def test_sizes_at_the_launch_edges(mod, n):
    check_host(mod, cube(n, 100 + n), 0.11)


def test_each_point_its_own_voxel(mod):
    xyz = cube(4097, 1)
    want = restate(xyz, 1e-4)
    assert want[0].shape[0] == 4097
    check_host(mod, xyz, 1e-4, want=want)


def test_all_points_in_one_voxel(mod):
    xyz = cube(5000, 2)
    want = restate(xyz, 10.0)
    assert want[0].shape[0] == 1 and want[1][0] == 5000
    check_host(mod, xyz, 10.0, want=want)


@pytest.mark.parametrize("v", [0.1, 0.0042])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_division_not_reciprocal(mod, axis, v):
    xyz = division_cloud(axis, v)
    assert xyz.min(axis=0)[axis] - 0.5 * v == 0.0
    a, b = cells(xyz, v), cells(xyz, v, reciprocal=True)
    assert (a != b).any(), "the two forms agree on this input: the test could not fail"
    by_div, by_rcp = restate(xyz, v), restate(xyz, v, reciprocal=True)
    assert not (by_div[0].shape == by_rcp[0].shape and same(by_div[0], by_rcp[0]))
    check_host(mod, xyz, v, want=by_div)


def test_exact_boundary_ties(mod):
    xyz = tie_cloud()
    assert (xyz < 0).any() and np.array_equal(xyz * 8, np.round(xyz * 8))
    q = (xyz - (xyz.min(axis=0) - 0.125)) / 0.25
    assert np.array_equal(q * 2, np.round(q * 2)) and (q == np.round(q)).any() and (q != np.round(q)).any()
    check_host(mod, xyz, 0.25)


def test_large_offsets(mod):
    check_host(mod, utm_cloud(), 0.1)


def test_sparse_grid_wide_key(mod):
    xyz = sparse_cloud()
    want = restate(xyz, 1.0)
    assert cells(xyz, 1.0).max(axis=0).tolist() == [(1 << 20) - 1] * 3  # 60 key bits
    assert 1900 < want[0].shape[0] <= 2048 and want[1].max() >= 4
    check_host(mod, xyz, 1.0, want=want)


@pytest.mark.parametrize("counts", [[31, 33, 1, 32, 34], [2047, 2049, 5, 2048, 40], [3000, 1, 2500, 33, 32]])
def test_counts_at_the_path_thresholds(mod, counts):
    """Voxels of exactly 32 / 33 and 2,048 / 2,049 points: the lane, LDS and compaction paths."""
    xyz = count_cloud(counts, 5)
    want = restate(xyz, 1.0)
    assert sorted(want[1].tolist()) == sorted([counts[0] + 1] + counts[1:])
    check_host(mod, xyz, 1.0, want=want)


def test_many_middle_sized_voxels(mod):
    xyz = cube(20000, 6)
    want = restate(xyz, 0.34)
    assert want[1].min() > 32 and want[1].max() < 2048 and want[0].shape[0] == 64
    check_host(mod, xyz, 0.34, want=want)


def test_shuffled_input(mod, bunny_unique):
    assert bunny_unique.shape == (34834, 3)
    a = check_host(mod, bunny_unique, 0.0042)
    perm = np.random.default_rng(14).permutation(bunny_unique.shape[0])
    b = check_host(mod, np.ascontiguousarray(bunny_unique[perm]), 0.0042)
    assert a[0].shape == b[0].shape and not same(a[0], b[0])  # other input order, other sums


# ------------------------------------------------------------------ batches
def batch_clouds(bunny_unique):
    return [(cube(1025, 21), 0.11), (cube(5000, 2), 10.0), (division_cloud(1, 0.0042), 0.0042), (tie_cloud(), 0.25),
            (utm_cloud(), 0.1), (sparse_cloud(), 1.0), (cube(1, 22), 0.3), (count_cloud([2047, 2049, 5, 2048, 40], 5), 1.0),
            (bunny_unique, 0.0042), (cube(63, 23), 0.05)]


def run_device(mod, clouds, device=0, with_lists=True):
    import torch
    xyz = np.concatenate([c for c, _ in clouds])
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c, _ in clouds])])
    d = torch.from_numpy(xyz).to("cuda")
    out = torch.full_like(d, float("nan"))
    cnt = torch.full((xyz.shape[0],), -7, dtype=torch.int32, device="cuda")
    fst = torch.full((xyz.shape[0],), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    out_off = mod.voxel_downsample_device(d.data_ptr(), off, [v for _, v in clouds], out.data_ptr(), device=device,
                                          count_ptr=cnt.data_ptr() if with_lists else 0,
                                          first_ptr=fst.data_ptr() if with_lists else 0)
    return out_off, out.cpu().numpy(), cnt.cpu().numpy(), fst.cpu().numpy()


@pytest.fixture(scope="module")
def lone(mod, bunny_unique):
    """Every batch cloud's lone host-entry result (checked against the restatement above)."""
    return [mod.voxel_downsample(c, v, return_counts=True) for c, v in batch_clouds(bunny_unique)]


@pytest.mark.parametrize("device,rounds", [(0, 2), (1 << 8, 1)])
def test_batch_independence(mod, bunny_unique, lone, device, rounds):
    clouds = batch_clouds(bunny_unique)
    assert len({c.shape[0] for c, _ in clouds}) > 5 and len({v for _, v in clouds}) > 5
    want_off = np.concatenate([[0], np.cumsum([r[0].shape[0] for r in lone])]).tolist()
    for rnd in range(rounds):  # (a second call on the same engine: no stale table or counter)
        use = clouds if rnd == 0 else clouds[::-1]
        ref = lone if rnd == 0 else lone[::-1]
        w_off = want_off if rnd == 0 else np.concatenate([[0], np.cumsum([r[0].shape[0] for r in ref])]).tolist()
        out_off, out, cnt, fst = run_device(mod, use, device=device)
        assert out_off == w_off
        for c, r in enumerate(ref):
            a, b = out_off[c], out_off[c + 1]
            assert same(out[a:b], r[0]), c
            assert same(cnt[a:b], r[1]) and same(fst[a:b], r[2]), c
        assert np.isnan(out[out_off[-1]:]).all() and (cnt[out_off[-1]:] == -7).all()  # nothing past the end
    out_off, out, cnt, fst = run_device(mod, clouds, device=device, with_lists=False)
    assert out_off == want_off and same(out[:out_off[-1]], np.concatenate([r[0] for r in lone]))
    assert (cnt == -7).all() and (fst == -7).all()


# ------------------------------------------------------------------ into registration
def _bytes(r):
    return (r.T.tobytes(), r.num_iterations, r.num_pure_se3_iterations, r.status)


def half_voxel(cloud):
    """A voxel size that keeps roughly half of the cloud's points (by the restatement)."""
    ext = float((cloud.max(axis=0) - cloud.min(axis=0)).max())
    best = None
    for v in ext * np.geomspace(1e-3, 0.2, 40):
        m = np.unique(cells(cloud, v), axis=0).shape[0]
        if best is None or abs(m - cloud.shape[0] / 2) < abs(best[1] - cloud.shape[0] / 2):
            best = (float(v), m)
    return best


def test_into_register_batch_device(mod, fixture_clouds):
    import torch
    src, tgt = fixture_clouds
    v, m = half_voxel(src)
    assert 0.3 * src.shape[0] < m < 0.7 * src.shape[0]
    params = mod.cli_params(number_of_nn_for_LRF=20)
    hs, ht = mod.voxel_downsample(src, v), mod.voxel_downsample(tgt, v)
    want = mod.register_batch([(hs, ht)], "se3_pt2pl", params)
    d = torch.from_numpy(np.concatenate([src, tgt])).to("cuda")
    out = torch.empty_like(d)
    torch.cuda.synchronize()
    out_off = mod.voxel_downsample_device(d.data_ptr(), [0, src.shape[0], src.shape[0] + tgt.shape[0]], v, out.data_ptr())
    assert out_off == [0, hs.shape[0], hs.shape[0] + ht.shape[0]]
    got = mod.register_batch_device(out.data_ptr(), out_off[0:2], out.data_ptr(), [out_off[1], out_off[2]], "se3_pt2pl", params)
    assert _bytes(got[0]) == _bytes(want[0])
    assert want[0].status == 0


def test_register_sequence_with_voxel_size(mod, bunny_unique):
    from se3icp import datasets
    clouds = []
    for seed in (2, 3):
        s, t, _ = datasets.bunny_pair(bunny_unique, seed=seed, subsample=0.2)
        clouds += [np.ascontiguousarray(s, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64)]
    clouds = clouds[:3]
    v = half_voxel(clouds[0])[0]
    params = mod.cli_params(number_of_nn_for_LRF=20)
    down = [mod.voxel_downsample(c, v) for c in clouds]
    assert all(0.2 * c.shape[0] < d.shape[0] < 0.8 * c.shape[0] for c, d in zip(clouds, down))
    want = mod.register_sequence(down, "se3_gicp", params)
    got = mod.register_sequence(clouds, "se3_gicp", params, voxel_size=v)
    assert [_bytes(r) for r in got] == [_bytes(r) for r in want]
    plain = mod.register_sequence(down, "se3_gicp", params, voxel_size=None)
    assert [_bytes(r) for r in plain] == [_bytes(r) for r in want]


# ------------------------------------------------------------------ errors found on the device
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_input(mod, bad):
    from se3icp import _lib
    xyz = cube(100, 30)
    good = mod.voxel_downsample(xyz, 0.2, return_counts=True)
    broken = xyz.copy()
    broken[57, 1] = bad
    with pytest.raises(mod.Se3IcpError) as e:
        mod.voxel_downsample(broken, 0.2)
    assert e.value.code == _lib.ERR_NONFINITE
    again = mod.voxel_downsample(xyz, 0.2, return_counts=True)  # the engine is fine afterwards
    assert all(same(a, b) for a, b in zip(good, again))
    want = restate(xyz, 0.2)
    assert all(same(a, b) for a, b in zip(again, want))


def test_too_small_and_key_overflow(mod):
    from se3icp import _lib
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])
    with pytest.raises(mod.Se3IcpError) as e:  # extent / voxel > INT_MAX
        mod.voxel_downsample(xyz, 1e-10)
    assert e.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(mod.Se3IcpError) as e:  # 3 x 22 bits = 66 > 63
        mod.voxel_downsample(xyz, 1.0 / 3e6)
    assert e.value.code == _lib.ERR_INVALID_ARG
    got = mod.voxel_downsample(xyz, 1.0 / 2e6)  # 3 x 21 bits
    assert same(got, xyz)
    thin = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    assert same(mod.voxel_downsample(thin, 1e-9), thin)  # one axis of 30 bits, two of none


def test_size_only(mod):
    L = mod.load()
    xyz = cube(777, 31)
    dp = C.POINTER(C.c_double)
    m = L.se3icp_voxel_downsample(0, xyz.ctypes.data_as(dp), 777, 0.11, None, None, None)
    assert m == restate(xyz, 0.11)[0].shape[0]
