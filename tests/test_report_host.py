"""CPU tests of the registration report's host side: the argument checks of the four
se3icp_register_*_report entries (they run before the device is looked up), the loud failure
without a device, the object surface, the ctypes mirrors against the header's layout, and
se3-icp_amd/csrc/report.hpp built for the host (tests/report_host.cpp): the expansion of the
reduced moments into the information matrix against a direct long-double sum, and the
stop-reason rule over every branch of pair_close_iteration."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "se3-icp_amd", "csrc")
NO_SUCH_DEVICE = 200  # an ordinal no machine has: the calls below never reach a GPU


@pytest.fixture(scope="module")
def mod():
    import se3icp
    se3icp.load()
    return se3icp


class _Call:
    """One valid call of each entry with single knobs turned; returns the status."""

    def __init__(self, mod):
        from se3icp import _lib
        self.lib = _lib
        self.L = _lib.load()
        self.mod = mod
        rng = np.random.default_rng(0)
        self.src = rng.random((50, 3))
        self.tgt = rng.random((60, 3))
        self.idx = np.zeros(50, np.int32)
        self.dist = np.zeros(50)

    def opts(self, max_d=0.1, per_point=False):
        return self.lib.ReportOptions(max_d, self.idx.ctypes.data if per_point else None,
                                      self.dist.ctypes.data if per_point else None, 0, 0)

    def run(self, entry, n_src=50, n_tgt=60, method=5, opts="default", reports="default"):
        lib, L = self.lib, self.L
        dp = C.POINTER(C.c_double)
        if opts == "default":
            opts = self.opts()
        res = (lib.Result * 2)()
        rep = (lib.Report * 2)() if reports == "default" else None
        prm = self.mod.default_params()
        var = (lib.Params * 2)(self.mod.default_params(alpha_rot=1.0), self.mod.default_params())
        op = C.byref(opts) if opts is not None else None
        if entry in ("batch", "sweep"):
            sp = (dp * 1)(self.src.ctypes.data_as(dp))
            tp = (dp * 1)(self.tgt.ctypes.data_as(dp))
            ns, nt = (C.c_int64 * 1)(n_src), (C.c_int64 * 1)(n_tgt)
            if entry == "batch":
                return L.se3icp_register_batch_report(NO_SUCH_DEVICE, 1, sp, ns, tp, nt, method, C.byref(prm), res, op, rep)
            return L.se3icp_register_sweep_report(NO_SUCH_DEVICE, 1, sp, ns, tp, nt, method, 2, var, 0, res, op, rep)
        ptr = C.c_void_p(4096)  # never dereferenced: no device is reached
        so, to = (C.c_int64 * 2)(0, n_src), (C.c_int64 * 2)(0, n_tgt)
        if entry == "batch_device":
            return L.se3icp_register_batch_report_device(NO_SUCH_DEVICE, 1, ptr, so, ptr, to, method, C.byref(prm), res,
                                                         None, op, rep)
        return L.se3icp_register_sweep_report_device(NO_SUCH_DEVICE, 1, ptr, so, ptr, to, method, 2, var, 0, res, None,
                                                     op, rep)


ENTRIES = ["batch", "batch_device", "sweep", "sweep_device"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_checks_come_before_the_device(mod, entry):
    from se3icp import _lib
    c = _Call(mod)
    assert c.run(entry, reports=None) == _lib.ERR_INVALID_ARG
    assert c.run(entry, opts=None) == _lib.ERR_INVALID_ARG
    assert c.run(entry, opts=c.opts(max_d=float("nan"))) == _lib.ERR_INVALID_ARG
    assert c.run(entry, n_src=0) == _lib.ERR_EMPTY_CLOUD
    assert c.run(entry, n_tgt=0) == _lib.ERR_EMPTY_CLOUD
    assert c.run(entry, method=10) == _lib.ERR_INVALID_METHOD
    assert c.run(entry, method=-1) == _lib.ERR_INVALID_METHOD
    # per-point buffers: a batch takes them, a sweep does not
    want = _lib.ERR_INVALID_ARG if entry.startswith("sweep") else _lib.ERR_NO_DEVICE
    assert c.run(entry, opts=c.opts(per_point=True)) == want
    # a valid call, every distance-limit convention included: no device, and no CPU fallback
    for d in (0.1, 0.0, -1.0, float("inf")):
        assert c.run(entry, opts=c.opts(max_d=d)) == _lib.ERR_NO_DEVICE
    for m in range(10):
        assert c.run(entry, method=m) == _lib.ERR_NO_DEVICE


def _plain_call(mod, entry, n_pairs=1, null=None, n_src=50, n_tgt=60, method=5, k_lrf=30):
    """One valid call of a non-report entry with single knobs turned; returns the status.
    null: the name of one pointer argument passed as NULL ("src0" / "tgt0": the first pair's
    cloud in a host entry's pointer array)."""
    from se3icp import _lib
    L = _lib.load()
    dp = C.POINTER(C.c_double)
    c = _Call(mod)
    res = (_lib.Result * 2)()
    prm = mod.default_params(number_of_nn_for_LRF=k_lrf)
    var = (_lib.Params * 2)(mod.default_params(number_of_nn_for_LRF=k_lrf, alpha_rot=1.0), prm)
    if entry in ("batch", "sweep"):
        a = {"src": (dp * 1)(None if null == "src0" else c.src.ctypes.data_as(dp)), "n_src": (C.c_int64 * 1)(n_src),
             "tgt": (dp * 1)(None if null == "tgt0" else c.tgt.ctypes.data_as(dp)), "n_tgt": (C.c_int64 * 1)(n_tgt)}
    else:
        a = {"src": C.c_void_p(4096), "n_src": (C.c_int64 * 2)(0, n_src),  # never dereferenced: no device is reached
             "tgt": C.c_void_p(4096), "n_tgt": (C.c_int64 * 2)(0, n_tgt)}
    a.update(params=C.byref(prm), variants=var, results=res)
    if null in a:
        a[null] = None
    if entry == "batch":
        return L.se3icp_register_batch(NO_SUCH_DEVICE, n_pairs, a["src"], a["n_src"], a["tgt"], a["n_tgt"], method,
                                       a["params"], a["results"])
    if entry == "batch_device":
        return L.se3icp_register_batch_device(NO_SUCH_DEVICE, n_pairs, a["src"], a["n_src"], a["tgt"], a["n_tgt"],
                                              method, a["params"], a["results"], None)
    if entry == "sweep":
        return L.se3icp_register_sweep(NO_SUCH_DEVICE, n_pairs, a["src"], a["n_src"], a["tgt"], a["n_tgt"], method, 2,
                                       a["variants"], 0, a["results"])
    return L.se3icp_register_sweep_device(NO_SUCH_DEVICE, n_pairs, a["src"], a["n_src"], a["tgt"], a["n_tgt"], method,
                                          2, a["variants"], 0, a["results"], None)


# (knobs of _plain_call, the status of the two sweep entries); the plain batch entries look the
# device up before anything else and answer every row with ERR_NO_DEVICE
_PLAIN_ROWS = [
    (dict(), "NO_DEVICE"),
    (dict(n_pairs=0), "INVALID_ARG"),
    (dict(n_pairs=-1), "INVALID_ARG"),
    (dict(null="src"), "INVALID_ARG"),
    (dict(null="n_src"), "INVALID_ARG"),
    (dict(null="tgt"), "INVALID_ARG"),
    (dict(null="n_tgt"), "INVALID_ARG"),
    (dict(null="results"), "INVALID_ARG"),
    (dict(null="variants"), "INVALID_ARG"),  # (a batch's params: NULL means the defaults)
    (dict(n_src=0), "EMPTY_CLOUD"),
    (dict(n_tgt=0), "EMPTY_CLOUD"),
    (dict(method=-1), "INVALID_METHOD"),
    (dict(method=10), "INVALID_METHOD"),
    (dict(method=5, k_lrf=0), "INVALID_ARG"),
    (dict(method=2, k_lrf=0), "NO_DEVICE"),
]


@pytest.mark.parametrize("entry", ENTRIES)
def test_status_table_of_the_plain_entries(mod, entry):
    """The status of every bad call of the four entries without a report, on a device ordinal
    no machine has: the sweeps check their arguments first, se3icp_register_batch and
    se3icp_register_batch_device look the device up first and leave the checks to the engine."""
    from se3icp import _lib
    rows = list(_PLAIN_ROWS)
    if entry in ("batch", "sweep"):
        rows += [(dict(null="src0"), "INVALID_ARG"), (dict(null="tgt0"), "INVALID_ARG")]
    for knobs, want in rows:
        if entry.startswith("batch"):
            want = "NO_DEVICE"
            if knobs.get("null") == "variants":
                knobs = dict(null="params")
        assert _plain_call(mod, entry, **knobs) == getattr(_lib, "ERR_" + want), (entry, knobs)


def test_python_entries_fail_loudly_without_a_device(mod):
    from se3icp import _lib
    a = np.random.default_rng(1).random((40, 3))
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_batch_report([(a, a)], "se3_pt2pl", device=NO_SUCH_DEVICE, max_correspondence_distance=0.1,
                                  per_point=True)
    assert e.value.code == _lib.ERR_NO_DEVICE
    variants = mod.sweep_params(mod.default_params(), alpha_rot=[1.0, 2.0])
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_sweep_report([(a, a)], "se3_pt2pl", variants, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_batch_report([(a, a)], "se3_pt2pl", device=NO_SUCH_DEVICE,
                                  max_correspondence_distance=float("nan"))
    assert e.value.code == _lib.ERR_INVALID_ARG


def test_versions(mod):
    L = mod.load()
    assert L.se3icp_report_version() == 1
    assert L.se3icp_abi_version() == 4


def test_object_surface(mod):
    from se3icp import _lib
    L = mod.load()
    reg = mod.IterativeSE3Registration()
    rep = _lib.Report()
    assert L.se3icp_get_report(reg._h, C.byref(rep)) == _lib.ERR_INVALID_ARG  # none requested
    with pytest.raises(mod.Se3IcpError) as e:
        reg.report
    assert e.value.code == _lib.ERR_INVALID_ARG
    assert L.se3icp_request_report(None, None) == _lib.ERR_INVALID_ARG
    bad = _lib.ReportOptions(float("nan"), None, None, 0, 0)
    assert L.se3icp_request_report(reg._h, C.byref(bad)) == _lib.ERR_INVALID_ARG
    reg.setSourceCloud(np.zeros((7, 3)))
    reg.request_report(0.25, per_point=True)
    assert reg._rep_bufs[0].shape == (7,) and reg._rep_bufs[1].shape == (7,)
    # requested, but no run has produced one yet
    assert L.se3icp_get_report(reg._h, C.byref(rep)) == _lib.ERR_INVALID_ARG
    assert L.se3icp_get_report(reg._h, None) == _lib.ERR_INVALID_ARG
    assert L.se3icp_request_report(reg._h, None) == 0  # withdrawn


@pytest.fixture(scope="module")
def host_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("rep") / "report_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "report_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    return out.returncode, [ln.split() for ln in out.stdout.strip().splitlines()]


def test_ctypes_mirrors_match_the_header(host_report):
    from se3icp import _lib
    _, lines = host_report
    mirrors = {"se3icp_report_options": _lib.ReportOptions, "se3icp_report": _lib.Report}
    sizes = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "sizeof"}
    offsets = {ln[1]: int(ln[2]) for ln in lines if ln[0] == "offset"}
    assert set(sizes) == set(mirrors)
    seen = 0
    for name, cls in mirrors.items():
        assert C.sizeof(cls) == sizes[name], name
        for field, _ in cls._fields_:
            assert getattr(cls, field).offset == offsets[f"{name}.{field}"], (name, field)
            seen += 1
    assert seen == len(offsets) == 13
    stop = [ln for ln in lines if ln[0] == "stop_values"][0]
    assert [int(x) for x in stop[1:]] == [_lib.STOP_CONVERGED, _lib.STOP_MAX_ITERATIONS, _lib.STOP_MAX_SE3_ITERATIONS,
                                          _lib.STOP_RUNAWAY]


def test_distance_limit_conventions_and_depth(host_report):
    _, lines = host_report
    ai = [ln for ln in lines if ln[0] == "all_inliers"][0]
    assert [int(x) for x in ai[1:]] == [1, 1, 1, 0, 1]  # 0, -1, +inf, 0.5, -inf
    # 6 (wave) + 2 (block) + chain + 3 + 18 for 1, 144, 145 and 17 blocks
    depth = [ln for ln in lines if ln[0] == "depth"][0]
    assert [int(x) for x in depth[1:]] == [30, 30, 31, 30]


EXPAND_CASES = [f"n{n}_c{c}_{s}" for n in (1, 2, 1000) for c in (0, 1) for s in ("s0.01", "s3", "raw")] + ["empty"]


@pytest.mark.parametrize("case", EXPAND_CASES)
def test_information_expansion(host_report, case):
    """|information - long-double sum G^T G| <= 4 (0 + 3 + 8) 2^-53 sum |term| per entry (the
    moments enter rounded once: depth 0), exact zeros where G^T G has no term."""
    _, lines = host_report
    got = [ln for ln in lines if ln[0] == "expand" and ln[1] == case]
    assert len(got) == 1 and got[0][2] == "ok", got


STOP_ROWS = ["icp_cap", "icp_criterion", "icp_both", "icp_neither", "icp_runaway", "icp_sf_unused", "pure_cap",
             "pure_criterion", "pure_both", "pure_neither", "pure_runaway", "se3_switch_cap", "se3_switch_change",
             "se3_no_switch", "se3_unswitched_runaway", "se3_cap", "se3_criterion", "se3_both", "se3_neither",
             "se3_runaway", "se3_cap_passed_by", "cf_cap", "cf_criterion"]


@pytest.mark.parametrize("row", STOP_ROWS)
def test_stop_reason_table(host_report, row):
    _, lines = host_report
    got = [ln for ln in lines if ln[0] == "stop" and ln[1] == row]
    assert len(got) == 1 and got[0][2] == "ok", got


def test_host_program(host_report):
    rc, lines = host_report
    assert rc == 0, lines
    assert int([ln for ln in lines if ln[0] == "stop_rows"][0][1]) == len(STOP_ROWS)
    assert len([ln for ln in lines if ln[0] == "expand"]) == len(EXPAND_CASES)
