"""The setup's per-point arrays as the loop consumes them (se3icp_set_setup_record): xyz64, the
weighted SE(3) rows fr64, nrm64, conf64 and the pair's setup scalars, read at the end of every
entry's setup.

A. Against references, inside a batch, through the host and the device entry.  Inputs, references
   and bars: setup_record_cases.py (the bars are derived there; test_setup_record_host.py holds the
   oracle to them on the same inputs).  The frames and normals are held to the long-double
   restatement of lrf_reference.py evaluated on the RECORDED normalized points, at the bars of
   test_gpu_frames.py (BAR_FACTOR times the oracle's maxima of the same run, no point excused).
   Weights: k_lrf8.hip, k_knn.hip and k_knn_big.hip (and k_sweep.hip) all form the row as
   al * x, al * y, al * z, be * q from finished axes -- the weight is the last operation, a lone
   product that nothing can contract with -- so the weighted rows are held to fl(alpha r),
   fl(beta t) of the rows recorded at alpha = beta = 1 bit for bit, in every kernel.

B. The record is bitwise the same wherever and however the pair is set up: every array and scalar
   compared as bytes, alone against every index of a mixed-size batch (host, device, an engine
   slot, the caller's stream), across the kernel choices, the sharing / seeding / taking / tree
   modes of a device batch (each run asserting from the call's statistics that the recorded class
   really was shared, seeded, taken or redone), on the tie inputs, graph against batch, posed
   against moved, sweep against batch.

Stated departures, where a comparison is not of everything: the confidences of a posed source
under se3_gicp_with_cf come from the raw z (se3icp.h, initial poses), so under a tilted pose the
source's conf is compared with the raw cloud's and everything else with the moved cloud's.
"""
import contextlib
import functools

import numpy as np
import pytest

import lrf_reference as L
import setup_record_cases as S
from lrf_reference import BAR_FACTOR, EPS

pytestmark = pytest.mark.gpu

ARRAYS = ("xyz", "rows", "normals", "conf")
SCALARS = ("norm_center", "norm_scale", "f32_center", "alpha", "beta", "n")
LOW = dict(max_num_iterations=2, max_num_se3_iterations=1)
SLOT1 = 0 | 1 << 8


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


@pytest.fixture(scope="module")
def scans():
    from se3icp import datasets
    s, _ = datasets.kitti_like_sequence(5, seed=4, n_az=200)
    return [np.ascontiguousarray(x, dtype=np.float64) for x in s]


@pytest.fixture(scope="module")
def mixed(bunny_unique):
    """Generic clouds of different sizes: a 40-point one, and 3,001 .. 6,145 points."""
    from se3icp import datasets
    out = []
    for seed, sub in ((2, 0.1), (3, 0.1), (5, 0.19)):
        src, tgt, _ = datasets.bunny_pair(bunny_unique, seed=seed, subsample=sub)
        out += [src, tgt]
    c = [np.ascontiguousarray(x, dtype=np.float64) for x in out]
    assert min(x.shape[0] for x in c[4:]) >= 6145
    return {"c40": c[0][100:140].copy(), "a": c[0], "b": c[1], "c": c[2][:3001].copy(), "d": c[3],
            "e": c[4][:6145].copy(), "f": c[5][:4097].copy()}


class DeviceBatch:
    """The pairs' clouds in two device buffers (sources, targets), every use a copy of its own."""

    def __init__(self, pairs, stream=None):
        import torch
        self.src_off = np.concatenate([[0], np.cumsum([s.shape[0] for s, _ in pairs])])
        self.tgt_off = np.concatenate([[0], np.cumsum([t.shape[0] for _, t in pairs])])
        src = np.ascontiguousarray(np.concatenate([s for s, _ in pairs]), dtype=np.float64)
        tgt = np.ascontiguousarray(np.concatenate([t for _, t in pairs]), dtype=np.float64)
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            self.d_src, self.d_tgt = torch.from_numpy(src).to("cuda"), torch.from_numpy(tgt).to("cuda")
        (stream.synchronize() if stream is not None else torch.cuda.synchronize())

    def args(self):
        return self.d_src.data_ptr(), self.src_off, self.d_tgt.data_ptr(), self.tgt_off


def record(mod, p, n_src, n_tgt, call, device=0):
    """The setup record of result slot p of the one registration `call` makes, and what it returns."""
    with mod.setup_record(p, n_src, n_tgt, device) as rec:
        res = call()
    return rec, res


def record_batch(mod, pairs, p, method, params, entry="host", device=0):
    ns, nt = pairs[p][0].shape[0], pairs[p][1].shape[0]
    if entry == "host":
        return record(mod, p, ns, nt, lambda: mod.register_batch(pairs, method, params, device), device)
    stream = None
    if entry == "stream":
        import torch
        stream = torch.cuda.Stream()
    batch = DeviceBatch(pairs, stream)
    out = record(mod, p, ns, nt, lambda: mod.register_batch_device(
        *batch.args(), method, params, device=device, stream=stream.cuda_stream if stream else 0), device)
    if stream:
        stream.synchronize()
    return out


def as_bytes(rec):
    out = {}
    for side in ("src", "tgt"):
        for k in ARRAYS:
            out[f"{side}.{k}"] = None if rec[side][k] is None else rec[side][k].tobytes()
        for k in SCALARS:
            out[f"{side}.{k}"] = np.asarray(rec[side][k], dtype=np.float64).tobytes()
    return out


def differing(a, b, skip=()):
    a, b = as_bytes(a), as_bytes(b)
    return [k for k in a if k not in skip and a[k] != b[k]]


def written(rec):
    return {side: tuple(k for k in ARRAYS if rec[side][k] is not None) for side in ("src", "tgt")}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ============================================================================ A. references
def check_normalization(rec, res, src, tgt, scale_pre, exact):
    """The recorded centres, scale and coordinates of one pair; returns (largest centre deviation in
    units of its bar -- 0 when it is exact --, scale deviation in units of its bar)."""
    cs, ct = rec["src"]["norm_center"], rec["tgt"]["norm_center"]
    cdev = 0.0
    for cloud, c in ((src, cs), (tgt, ct)):
        if exact:
            assert np.array_equal(bits(c), bits(S.center_exact(cloud))), (c, S.center_exact(cloud))
        else:
            d = (np.abs(c.astype(S.LD) - S.center_ld(cloud)) / S.center_bound(cloud, c)).astype(np.float64)
            cdev = max(cdev, float(d.max()))
            assert (d <= 1.0).all(), (cloud.shape[0], d)
    s = rec["src"]["norm_scale"]
    assert np.float64(s).tobytes() == np.float64(rec["tgt"]["norm_scale"]).tobytes()
    assert np.float64(s).tobytes() == np.float64(res.scaling_factor).tobytes()
    s_ld, _ = S.scale_ld(src, tgt, cs, ct, scale_pre)
    sdev = S.scale_deviation(s, s_ld)
    assert sdev <= 1.0, (s, float(s_ld), sdev)
    for side, cloud, c in (("src", src, cs), ("tgt", tgt, ct)):
        assert rec[side]["n"] == cloud.shape[0]
        assert np.array_equal(bits(rec[side]["xyz"]), bits(S.normalized(cloud, c, s))), side
        assert not rec[side]["f32_center"].any()
    return cdev, sdev


@pytest.mark.parametrize("entry", ["host", "device"])
def test_normalization_at_the_chunk_edges(se3icp_mod, parity_record, entry):
    """2,047 .. 6,145 points, exact sums: the centre is fsum / n bit for bit and the scale within
    8 * 2^-53 of the long-double one about the recorded centres, the pair's farthest point being
    the last point of the target's (pairs 0, 2) or the source's (pairs 1, 3) last chunk."""
    pairs = S.edge_pairs()
    prm = se3icp_mod.default_params(number_of_nn_for_LRF=10, **LOW)
    top = 0.0
    for p, (src, tgt) in enumerate(pairs):
        rec, res = record_batch(se3icp_mod, pairs, p, "se3_pt2pt", prm, entry)
        _, sdev = check_normalization(rec, res[p], src, tgt, prm.scale_preprocessing, exact=True)
        print(f"[setup record] edges {entry} pair {p} ({src.shape[0]}, {tgt.shape[0]}): scale off by {sdev:.3f} bars")
        top = max(top, sdev)
        assert written(rec) == {"src": ("xyz", "rows"), "tgt": ("xyz", "rows")}
    parity_record(f"setup record: chunk edges {entry}", pairs=len(pairs), centres_exact=True, scale_dev_bars=top)


def test_normalization_past_64_chunks(se3icp_mod, parity_record):
    """131,073 points, 65 chunks: lane 0 of k_pair_centers folds two chunks, the last of one point,
    which is the pair's farthest.  A cheap method and one iteration."""
    pairs = S.wrap_pairs()
    prm = se3icp_mod.default_params(number_of_nn_for_LRF=10, max_num_iterations=1, max_num_se3_iterations=1)
    top = 0.0
    for p, entry in ((0, "host"), (1, "host"), (1, "device")):
        rec, res = record_batch(se3icp_mod, pairs, p, "se3_pt2pt", prm, entry)
        _, sdev = check_normalization(rec, res[p], pairs[p][0], pairs[p][1], prm.scale_preprocessing, exact=True)
        print(f"[setup record] wrap {entry} pair {p}: scale off by {sdev:.3f} bars")
        top = max(top, sdev)
    parity_record("setup record: 65 chunks", pairs=len(pairs), centres_exact=True, scale_dev_bars=top)


@pytest.mark.parametrize("entry", ["host", "device"])
def test_normalization_off_origin(se3icp_mod, parity_record, entry):
    """Generic coordinates at UTM-sized offsets: the centre within the any-order summation bound,
    the scale and the coordinates as above."""
    pairs = S.utm_pairs()
    prm = se3icp_mod.default_params(number_of_nn_for_LRF=10, **LOW)
    tc = ts = 0.0
    for p, (src, tgt) in enumerate(pairs):
        rec, res = record_batch(se3icp_mod, pairs, p, "se3_pt2pt", prm, entry)
        cdev, sdev = check_normalization(rec, res[p], src, tgt, prm.scale_preprocessing, exact=False)
        print(f"[setup record] utm {entry} pair {p}: centre off by {cdev:.4f} bounds, scale by {sdev:.3f} bars")
        tc, ts = max(tc, cdev), max(ts, sdev)
    parity_record(f"setup record: off origin {entry}", pairs=len(pairs), centre_dev_bounds=tc, scale_dev_bars=ts)


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("method", ["pt2pt", "pt2pl", "gicp"])
def test_run_icp_records_the_input(se3icp_mod, method, entry):
    """run_icp keeps raw coordinates: the recorded xyz is the input bit for bit, no rows, the
    normals the method estimates, centre 0 and scale 1; the f32 centre is the target's."""
    pairs = S.utm_pairs()
    prm = se3icp_mod.default_params(**LOW)
    want = {"pt2pt": ((), ()), "pt2pl": ((), ("normals",)), "gicp": (("normals",), ("normals",))}[method]
    for p, (src, tgt) in enumerate(pairs):
        rec, res = record_batch(se3icp_mod, pairs, p, method, prm, entry)
        assert written(rec) == {"src": ("xyz",) + want[0], "tgt": ("xyz",) + want[1]}
        for side, cloud in (("src", src), ("tgt", tgt)):
            assert np.array_equal(bits(rec[side]["xyz"]), bits(cloud)), (p, side)
            assert not rec[side]["norm_center"].any() and rec[side]["norm_scale"] == 1.0
            c = rec[side]["f32_center"]
            assert np.array_equal(bits(c), bits(rec["tgt"]["f32_center"]))
            assert (np.abs(c.astype(S.LD) - S.center_ld(tgt)) <= S.center_bound(tgt, c)).all()
        assert res[p].scaling_factor == 1.0


@pytest.mark.parametrize("entry", ["host", "device"])
def test_confidences(se3icp_mod, parity_record, entry):
    """conf against lounge_confidence of the RAW z in long double, z over [0.4, 4] with both ends."""
    pairs = S.depth_pairs()
    prm = se3icp_mod.default_params(number_of_nn_for_LRF=10, **LOW)
    top = 0.0
    for p, (src, tgt) in enumerate(pairs):
        rec, _ = record_batch(se3icp_mod, pairs, p, "se3_gicp_with_cf", prm, entry)
        assert written(rec) == {"src": ARRAYS, "tgt": ARRAYS}
        for side, cloud in (("src", src), ("tgt", tgt)):
            dev = S.conf_deviation(rec[side]["conf"], cloud[:, 2])
            top = max(top, float(dev.max()))
            assert (dev <= 1.0).all(), (p, side, float(dev.max()), int(dev.argmax()))
    print(f"[setup record] confidences {entry}: off by {top:.3f} bars at most")
    parity_record(f"setup record: confidences {entry}", pairs=len(pairs), conf_dev_bars=top)


@functools.lru_cache(maxsize=None)
def _ld_knn(xyz_bytes, n):
    return L.knn_ld(np.frombuffer(xyz_bytes, dtype=np.float64).reshape(n, 3), L.K_MAX)


@functools.lru_cache(maxsize=None)
def _ld_case(xyz_bytes, n, k, k_nrm):
    """(kNN lists, frame parts, normal reference) of recorded normalized points, once per cloud."""
    pts = np.frombuffer(xyz_bytes, dtype=np.float64).reshape(n, 3)
    idx = _ld_knn(xyz_bytes, n)
    return idx, L.toldi_z(pts, idx, k), (L.normals_ld(pts, idx, k_nrm) if k_nrm else None)


@pytest.fixture(scope="module")
def bars(refcpu):
    ora = L.oracle_maxima()
    return tuple(BAR_FACTOR * v for v in ora), ora


@pytest.mark.parametrize("k", S.FRAME_KS)
@pytest.mark.parametrize("method", ["se3_pt2pl", "se3_gicp"])
def test_frames_and_normals_of_designed_clouds(se3icp_mod, bars, parity_record, method, k):
    """The designed clouds of 517 and 4,099 points as source and target (and target and source) of
    one batch, alpha = beta = 1: the recorded frames and normals against the long-double
    restatement on the recorded normalized points, whose brute-force kNN lists are the raw clouds'."""
    (bz, bx, bn), ora = bars
    a, b = (L.cloud(kind) for kind in S.FRAME_KINDS)
    pairs = [(np.array(a), np.array(b)), (np.array(b), np.array(a))]
    prm = se3icp_mod.default_params(number_of_nn_for_LRF=k, alpha_rot=1.0, beta_transl=1.0, **LOW)
    k_nrm = {"se3_pt2pl": (0, 30), "se3_gicp": (20, 20)}[method]
    top = {"kz": 0.0, "kx": 0.0, "kn": 0.0, "ydev": 0.0}
    fails = []
    for p in (0, 1):
        rec, _ = record_batch(se3icp_mod, pairs, p, method, prm, "host" if p == 0 else "device")
        kinds = S.FRAME_KINDS if p == 0 else S.FRAME_KINDS[::-1]
        for side, kind, kn_k in zip(("src", "tgt"), kinds, k_nrm):
            r = rec[side]
            n = r["n"]
            assert (r["alpha"], r["beta"]) == (1.0, 1.0) and (r["normals"] is not None) == (kn_k > 0)
            idx, parts, nref = _ld_case(r["xyz"].tobytes(), n, k, kn_k)
            assert np.array_equal(idx, L.knn_of(kind)), (kind, "the scale created a tie")
            F = S.frames_of_rows(r["rows"])
            assert np.isfinite(F).all()
            kz, kx, ydev, zsv = L.frame_measures(parts, F)
            vals = [("kz", kz, bz), ("kx", kx, bx), ("ydev", ydev, 4 * EPS)]
            if kn_k:
                assert np.isfinite(r["normals"]).all()
                vals.append(("kn", L.normal_measure(nref, r["normals"]), bn))
            for key, val, bar in vals:
                top[key] = max(top[key], float(val.max()))
                if not val.max() <= bar:
                    fails.append((p, side, key, float(val.max()), int(val.argmax()), bar))
            if not (zsv >= 0).all():
                fails.append((p, side, "z sign", np.nonzero(zsv < 0)[0][:8].tolist()))
            if not np.array_equal(bits(r["rows"][:, 9:12]), bits(r["xyz"])):
                fails.append((p, side, "translation"))
    print(f"[setup record] frames {method} k={k}: K_z {top['kz']:.2f}  K_x {top['kx']:.2f}  K_n {top['kn']:.2f}  "
          f"(oracle {ora[0]:.2f} {ora[1]:.2f} {ora[2]:.2f})  |y - z x x| {top['ydev'] / EPS:.2f} eps")
    parity_record(f"setup record: frames {method} k={k}", K_z=top["kz"], K_x=top["kx"], K_n=top["kn"],
                  y_dev_eps=top["ydev"] / EPS, K_z_oracle=ora[0], K_x_oracle=ora[1], K_n_oracle=ora[2])
    assert not fails, fails


@pytest.mark.parametrize("exact", [0, 1, 2])
@pytest.mark.parametrize("method", ["se3_pt2pl", "se3_gicp_with_cf"])
def test_weighted_rows(se3icp_mod, parity_record, method, exact):
    """rows at (alpha, beta) = (0.5, 2) and (0.3, 3) are fl(alpha r), fl(beta t) of the rows at
    (1, 1), bit for bit, in k_lrf8 (0), k_lrf (1) and k_knn_big (2): each multiplies the finished
    axes and the point by the weight as its last operation.  A se3_gicp_with_cf target's f64 row
    keeps the weighted translation (only its f32 search row takes the point's)."""
    from se3icp import registration
    pairs = S.depth_pairs()
    p = 1
    registration.set_lrf_exact(exact)
    try:
        recs = {}
        for al, be in ((1.0, 1.0), (0.5, 2.0), (0.3, 3.0)):
            prm = se3icp_mod.default_params(number_of_nn_for_LRF=30, alpha_rot=al, beta_transl=be, **LOW)
            recs[(al, be)], _ = record_batch(se3icp_mod, pairs, p, method, prm, "host")
    finally:
        registration.set_lrf_exact(0)
    base = recs[(1.0, 1.0)]
    for (al, be), rec in recs.items():
        for side in ("src", "tgt"):
            r0, r = base[side]["rows"], rec[side]["rows"]
            assert (rec[side]["alpha"], rec[side]["beta"]) == (al, be)
            assert np.array_equal(bits(r[:, :9]), bits(np.float64(al) * r0[:, :9])), (al, be, side, "rotation")
            assert np.array_equal(bits(r[:, 9:]), bits(np.float64(be) * r0[:, 9:])), (al, be, side, "translation")
            assert np.array_equal(bits(r0[:, 9:]), bits(base[side]["xyz"]))
        assert not differing(rec, base, skip=("src.rows", "tgt.rows", "src.alpha", "tgt.alpha", "src.beta", "tgt.beta"))
    parity_record(f"setup record: weights {method} exact {exact}", equal=True)


# ============================================================================ B. bitwise
def _others(m):
    return [(m["c40"], m["a"]), (m["b"], m["c"]), (m["d"], m["a"])]


@pytest.mark.parametrize("method", ["se3_gicp", "se3_gicp_with_cf", "gicp"])
def test_alone_against_every_index_of_a_mixed_batch(se3icp_mod, mixed, parity_record, method):
    """One pair (6,145 onto 4,097 points) alone and at every index of a batch that begins with a
    40-point source: host entry, device entry, a further engine slot, the caller's stream."""
    mod = se3icp_mod
    q = (mixed["e"], mixed["f"])
    prm = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    alone, _ = record_batch(mod, [q], 0, method, prm, "host")
    assert alone["src"]["n"] == 6145 and alone["tgt"]["n"] == 4097
    cases = [("alone device", [q], 0, "device", 0), ("alone slot 1", [q], 0, "host", SLOT1)]
    for i in range(4):
        batch = _others(mixed)[:i] + [q] + _others(mixed)[i:]
        cases += [(f"index {i} host", batch, i, "host", 0), (f"index {i} device", batch, i, "device", 0)]
    batch = _others(mixed)[:2] + [q] + _others(mixed)[2:]
    cases += [("index 2 slot 1 device", batch, 2, "device", SLOT1), ("index 2 stream", batch, 2, "stream", 0),
              ("index 2 slot 1 stream", batch, 2, "stream", SLOT1)]
    bad = {}
    for name, pairs, p, entry, device in cases:
        rec, _ = record_batch(mod, pairs, p, method, prm, entry, device)
        d = differing(rec, alone)
        if d:
            bad[name] = d
    print(f"[setup record] alone vs batch {method}: {len(cases)} placements, differing: {bad}")
    parity_record(f"setup record: placements {method}", placements=len(cases), equal=not bad)
    assert not bad, bad


@pytest.mark.parametrize("method", ["se3_gicp", "se3_pt2pl"])
@pytest.mark.parametrize("k", [30, 150])
def test_kernel_choices(se3icp_mod, mixed, parity_record, method, k):
    """se3icp_set_lrf_exact 0 / 1 / 2 (1 holds k <= 128 only)."""
    from se3icp import registration
    pairs = _others(mixed)[:2] + [(mixed["e"], mixed["f"])]
    prm = se3icp_mod.default_params(number_of_nn_for_LRF=k, **LOW)
    recs = {}
    for mode in (0, 1, 2) if k <= 128 else (0, 2):
        registration.set_lrf_exact(mode)
        try:
            recs[mode] = [record_batch(se3icp_mod, pairs, p, method, prm, "host")[0] for p in (0, 2)]
        finally:
            registration.set_lrf_exact(0)
    bad = {(mode, i): differing(r, recs[0][i]) for mode, rr in recs.items() for i, r in enumerate(rr)
           if differing(r, recs[0][i])}
    parity_record(f"setup record: kernels {method} k={k}", modes=len(recs), equal=not bad)
    assert not bad, bad


@contextlib.contextmanager
def engine_modes(mod, sharing=0, seeding=0, taking=0, tree=0, device=0):
    mod.set_batch_sharing(sharing, device)
    mod.set_lrf_seeding(seeding, device)
    mod.set_lrf_taking(taking, device)
    mod.set_tree_sharing(tree, device)
    try:
        yield
    finally:
        mod.set_batch_sharing(0, device)
        mod.set_lrf_seeding(0, device)
        mod.set_lrf_taking(0, device)
        mod.set_tree_sharing(0, device)


def record_modes(mod, pairs, p, method, prm, **modes):
    """Pair p of the device batch under the given engine modes: (record, graph, seed, take, tree stats)."""
    ns, nt = pairs[p][0].shape[0], pairs[p][1].shape[0]
    batch = DeviceBatch(pairs)
    with engine_modes(mod, **modes):
        rec, _ = record(mod, p, ns, nt, lambda: mod.register_batch_device(*batch.args(), method, prm))
        return rec, mod.last_graph_stats(), mod.last_seed_stats(), mod.last_take_stats(), mod.last_tree_stats()


NO_TAKES = {"classes_taking": 0, "queries_taken": 0, "queries_redone": 0, "queries_failed": 0}


@pytest.mark.parametrize("method", ["se3_gicp", "se3_gicp_with_cf"])
def test_chain_across_the_sharing_modes(se3icp_mod, scans, parity_record, method):
    """The five-scan chain as a device batch, its pairs in reverse order: slots s4 s3 | s3 s2 |
    s2 s1 | s1 s0.  Scans 3 and 2 run under two scales each and their SECOND class is the source of
    pairs 1 and 2; scan 1's two uses are one class, so the source of pair 3 is a k_graph_share
    copy.  Pairs 1 and 3 are recorded under every mode and compared with the plain batch
    (sharing level 1); the statistics of every run say what the recorded classes did."""
    mod = se3icp_mod
    pairs = mod.expand_edges(scans, mod.sequence_edges(5))[::-1]
    prm = mod.kitti_params(**LOW)
    n23 = scans[2].shape[0] + scans[3].shape[0]
    runs = [  # (name, modes, what the statistics must say)
        ("take", dict(sharing=2), "taken"),
        ("take, bounds halved", dict(sharing=2, taking=2), "redone"),
        ("seeded", dict(sharing=2, taking=1), "seeded"),
        ("seeds halved", dict(sharing=2, seeding=2), "seed failed"),
        ("seeds times 4", dict(sharing=2, seeding=3), "seeded"),
        ("unseeded", dict(sharing=2, seeding=1), "shared"),
        ("own trees", dict(sharing=2, tree=1), "seeded own trees"),
        ("own trees unseeded", dict(sharing=2, seeding=1, tree=1), "shared own trees"),
    ]
    bad = {}
    for p in (1, 3):
        plain, _, sd, tk, tr = record_modes(mod, pairs, p, method, prm, sharing=1)
        assert sd["classes_seeded"] == 0 and tk == NO_TAKES and tr["adopted_3d"] == 0, (sd, tk, tr)
        for name, modes, what in runs:
            rec, g, sd, tk, tr = record_modes(mod, pairs, p, method, prm, **modes)
            assert tuple(g.values()) == (5, 8, 7, 7, 0, 0, 0, 0, 0), (name, g)  # one class is shared
            if "own trees" in what:
                assert tr["adopted_3d"] == 0 and tr["adopted_12d"] == 0 and tk == NO_TAKES, (name, tr, tk)
            else:
                assert tr["adopted_3d"] == 3 and tr["adopted_12d"] == 3, (name, tr)
            if what.startswith("shared"):
                assert sd["classes_seeded"] == 0 and tk == NO_TAKES, (name, sd, tk)
            else:
                assert sd["classes_seeded"] == 2, (name, sd)  # the second classes of scans 3 and 2
                assert sd["queries_seeded"] + sd["queries_unseeded"] == n23, (name, sd)
            if what == "taken":
                assert tk["classes_taking"] == 2 and tk["queries_taken"] > 0.9 * n23 and tk["queries_failed"] == 0, tk
            if what == "redone":
                assert tk["classes_taking"] == 2 and tk["queries_taken"] == 0 and tk["queries_redone"] == n23, tk
            if what in ("seeded", "seed failed"):
                assert tk == NO_TAKES, (name, tk)
                assert (sd["queries_failed"] > 0) == (what == "seed failed"), (name, sd)
            d = differing(rec, plain)
            if d:
                bad[(p, name)] = d
    print(f"[setup record] chain {method}: {2 * len(runs)} runs against the plain batch, differing: {bad}")
    parity_record(f"setup record: chain modes {method}", runs=2 * len(runs), equal=not bad)
    assert not bad, bad


def _tie_cases(mod):
    lat = [S.lattice(11, 1.0), S.lattice(12, 1.0), S.lattice(10, 2.0)]
    gap = S.rounding_gap_clouds()
    return {"lattices": (mod.expand_edges(lat, [(1, 0), (2, 1), (0, 2), (0, 0)]), (1, 2, 3),
                         dict(number_of_nn_for_LRF=30, max_num_se3_iterations=4, max_num_iterations=12)),
            "rounding-level gap": (mod.expand_edges(gap, [(1, 0), (2, 1)]), (0, 1),
                                   dict(number_of_nn_for_LRF=30, max_num_se3_iterations=3, max_num_iterations=8))}


@pytest.mark.parametrize("name", ["lattices", "rounding-level gap"])
def test_tie_inputs_across_taking_and_seeding(se3icp_mod, parity_record, name):
    """Where the order of near-tied neighbours decides the order of the sums: the integer lattices
    and the two point-symmetric clusters, each with a cloud under two scales, recorded for the
    pairs that hold a second class, taking 0 / 1 / 2 and seeding 0 / 1 against the plain batch."""
    mod = se3icp_mod
    pairs, recorded, prm = _tie_cases(mod)[name]
    prm = mod.default_params(**prm)
    bad = {}
    redone = 0
    for p in recorded:
        plain, *_ = record_modes(mod, pairs, p, "se3_gicp", prm, sharing=1)
        for mname, modes in (("take", dict(sharing=2)), ("no take", dict(sharing=2, taking=1)),
                             ("halved", dict(sharing=2, taking=2)), ("unseeded", dict(sharing=2, seeding=1))):
            rec, g, sd, tk, _ = record_modes(mod, pairs, p, "se3_gicp", prm, **modes)
            assert g["classes"] > g["clouds"], g  # some cloud has a second class
            if mname == "unseeded":
                assert sd["classes_seeded"] == 0 and tk == NO_TAKES
            else:
                assert sd["classes_seeded"] > 0, sd
                assert (tk["classes_taking"] > 0) == (mname != "no take"), (mname, tk)
            if mname == "take":
                redone = max(redone, tk["queries_redone"])
            d = differing(rec, plain)
            if d:
                bad[(p, mname)] = d
    assert redone > 0  # (the ties do send wavefronts back)
    parity_record(f"setup record: ties {name}", pairs=len(recorded), equal=not bad)
    assert not bad, bad


@pytest.mark.parametrize("method", ["se3_gicp", "gicp"])
@pytest.mark.parametrize("shape", ["chain", "map"])
def test_graph_against_the_expanded_batch(se3icp_mod, scans, parity_record, shape, method):
    """register_graph (every sharing level) against register_batch on the expanded pair list."""
    mod = se3icp_mod
    if shape == "chain":
        clouds, edges = scans, mod.sequence_edges(5)
    else:
        clouds = [np.ascontiguousarray(s * f) for s, f in zip(scans, (1.5, 1.4, 1.0, 1.3, 1.2))]
        edges = [(0, 2), (1, 2), (3, 2), (4, 2)]
    pairs = mod.expand_edges(clouds, edges)
    prm = mod.kitti_params(**LOW)
    bad = {}
    for p in (1, 3):
        ns, nt = pairs[p][0].shape[0], pairs[p][1].shape[0]
        want, _ = record_batch(mod, pairs, p, method, prm, "host")
        for lv in (1, 2, 3):
            rec, _ = record(mod, p, ns, nt, lambda: mod.register_graph(clouds, edges, method, prm, sharing=lv))
            g = mod.last_graph_stats()
            assert g["uses"] == 8 and g["clouds"] == 5, g
            # something selected once for several uses (the map's scan 2 runs under four scales:
            # run_se3_* shares nothing there; run_icp selects once per cloud)
            assert g["classes_full"] < 8 or lv == 1 or (shape, method) == ("map", "se3_gicp"), g
            d = differing(rec, want)
            if d:
                bad[(p, lv)] = d
    parity_record(f"setup record: graph {shape} {method}", edges=len(edges), equal=not bad)
    assert not bad, bad


@pytest.mark.parametrize("method", ["se3_gicp", "se3_gicp_with_cf"])
@pytest.mark.parametrize("pose", ["z-preserving", "tilted"])
def test_posed_edge_against_the_moved_source(se3icp_mod, mixed, parity_record, pose, method):
    """register_graph with an initial pose on edge 0 against the plain graph on the source moved in
    numpy (apply_pose, no FMA).  se3_gicp_with_cf: the source's conf is the RAW cloud's; under the
    z-preserving pose that is the moved cloud's as well, under the tilted one it is compared with
    the raw cloud's record and everything else with the moved cloud's."""
    from test_gpu_init import np_apply, rigid
    mod = se3icp_mod
    if pose == "z-preserving":
        c, s = np.cos(0.03), np.sin(0.03)
        T0 = np.array([[c, -s, 0.0, 0.004], [s, c, 0.0, -0.003], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])
    else:
        T0 = rigid(0.05, -0.04, 0.3, [0.2, -0.1, 0.05])
    clouds = [mixed["a"], mixed["b"], mixed["c"]]
    edges = [(0, 1), (2, 1), (0, 2)]
    moved = np_apply(T0, clouds[0])
    assert (moved[:, 2].tobytes() == clouds[0][:, 2].tobytes()) == (pose == "z-preserving")
    prm = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    ns, nt = clouds[0].shape[0], clouds[1].shape[0]
    got, _ = record(mod, 0, ns, nt, lambda: mod.register_graph(clouds, edges, method, prm, init=[T0, None, None]))
    assert mod.last_init_stats()["posed_edges"] == 1
    want, _ = record(mod, 0, ns, nt, lambda: mod.register_graph(clouds + [moved], [(3, 1), (2, 1), (0, 2)], method, prm))
    skip = ()
    if method == "se3_gicp_with_cf" and pose == "tilted":
        skip = ("src.conf",)
        raw, _ = record(mod, 0, ns, nt, lambda: mod.register_graph(clouds, edges, method, prm))
        assert got["src"]["conf"].tobytes() == raw["src"]["conf"].tobytes()
        assert got["src"]["conf"].tobytes() != want["src"]["conf"].tobytes()
    d = differing(got, want, skip)
    parity_record(f"setup record: posed {pose} {method}", equal=not d)
    assert not d, d


@pytest.mark.parametrize("method", ["se3_gicp", "se3_gicp_with_cf", "gicp"])
def test_sweep_variant_against_the_batch(se3icp_mod, mixed, parity_record, method):
    """register_sweep at variant v (record index v * P + p; three variants in groups of two, so
    variant 2 is in the second group) against register_batch with variants[v]."""
    mod = se3icp_mod
    pairs = [(mixed["c40"], mixed["a"]), (mixed["e"], mixed["f"])]
    base = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    variants = mod.sweep_params(base, alpha_rot=[1.0, 0.5, 3.0], beta_transl=[1.0, 2.0, 0.7])
    P = len(pairs)
    bad = {}
    for v, p in ((0, 1), (1, 0), (1, 1), (2, 0), (2, 1)):
        ns, nt = pairs[p][0].shape[0], pairs[p][1].shape[0]
        got, _ = record(mod, v * P + p, ns, nt, lambda: mod.register_sweep(pairs, method, variants, max_group=2))
        want, _ = record_batch(mod, pairs, p, method, variants[v], "host")
        assert (want["src"]["alpha"], want["src"]["beta"]) == (variants[v].alpha_rot, variants[v].beta_transl)
        d = differing(got, want)
        if d:
            bad[(v, p)] = d
    parity_record(f"setup record: sweep {method}", variants=3, equal=not bad)
    assert not bad, bad


def test_arming_rules(se3icp_mod, mixed):
    """One-shot; an index outside the call's results is SE3ICP_ERR_INVALID_ARG from that call;
    arrays too small for the cloud likewise; an unarmed call records nothing."""
    import ctypes as C
    from se3icp import _lib
    mod = se3icp_mod
    pairs = [(mixed["c40"], mixed["a"])]
    prm = mod.default_params(number_of_nn_for_LRF=30, **LOW)
    with pytest.raises(_lib.Se3IcpError) as e:
        with mod.setup_record(1, 40, mixed["a"].shape[0]):
            mod.register_batch(pairs, "se3_gicp", prm)
    assert e.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(_lib.Se3IcpError) as e:
        with mod.setup_record(0, 39, mixed["a"].shape[0]):
            mod.register_batch(pairs, "se3_gicp", prm)
    assert e.value.code == _lib.ERR_INVALID_ARG
    rec = _lib.SetupRecord()
    rec.pair = 0  # no arrays: the scalars and the sizes alone
    _lib.check(_lib.load().se3icp_set_setup_record(0, C.byref(rec)))
    want = mod.register_batch(pairs, "se3_gicp", prm)
    assert rec.recorded == 1 and (rec.src.n, rec.tgt.n) == (40, mixed["a"].shape[0]) and rec.src.written == 0
    rec.recorded = 0
    again = mod.register_batch(pairs, "se3_gicp", prm)  # disarmed by the call before
    assert rec.recorded == 0 and again[0].T.tobytes() == want[0].T.tobytes()
