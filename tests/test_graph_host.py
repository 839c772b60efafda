"""CPU tests of the cloud-graph entries' host side: the argument checks of
se3icp_register_graph(_device, _report) (they run before the device is looked up, so a bad
call is reported as such on a host without a GPU), the loud failure without a device,
sequence_edges / expand_edges, and the class planning of se3-icp_amd/csrc/graph.hpp, built for
the host (tests/graph_host.cpp) as test_sweep_host.py builds sweep.hpp."""
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


def _call(n_pts=(50, 60, 70), src=(1, 2), tgt=(0, 1), method="se3_gicp", sharing=0, n_clouds=None, n_pairs=None,
          null=None, device=NO_SUCH_DEVICE, params="default"):
    """se3icp_register_graph with one knob turned; returns the status."""
    from se3icp import _lib
    L = _lib.load()
    nc = len(n_pts)
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(0)
    clouds = [rng.random((max(k, 1), 3)) for k in n_pts]
    cp = (dp * nc)(*[a.ctypes.data_as(dp) for a in clouds])
    cn = (C.c_int64 * nc)(*n_pts)
    es = (C.c_int32 * len(src))(*src)
    et = (C.c_int32 * len(tgt))(*tgt)
    res = (_lib.Result * max(1, len(src)))()
    mid = method if isinstance(method, int) else _lib.method_id(method)
    prm = _lib.default_params() if params == "default" else params
    args = dict(xyz=cp, n_pts=cn, src=es, tgt=et, results=res)
    if null:
        args[null] = None
    return L.se3icp_register_graph(device, nc if n_clouds is None else n_clouds, args["xyz"], args["n_pts"],
                                   len(src) if n_pairs is None else n_pairs, args["src"], args["tgt"], mid,
                                   C.byref(prm) if prm is not None else None, sharing, args["results"])


def test_valid_call_without_device_fails_loudly(mod):
    from se3icp import _lib
    assert _call() == _lib.ERR_NO_DEVICE
    a = np.random.default_rng(1).random((40, 3))
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_graph([a, a + 1.0], [(1, 0)], "se3_pt2pl", device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_sequence([a, a + 1.0, a], "gicp", device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_graph_report([a, a + 1.0], [(1, 0)], "se3_gicp", device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.last_graph_stats(device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    if mod.device_count() == 0:  # and on the default device of a host without one
        with pytest.raises(mod.Se3IcpError) as e:
            mod.register_graph([a, a + 1.0], [(1, 0)], "se3_pt2pl")
        assert e.value.code == _lib.ERR_NO_DEVICE


@pytest.mark.parametrize("case", ["n_clouds_zero", "n_clouds_negative", "n_pairs_zero", "n_pairs_negative", "xyz_null",
                                  "n_pts_null", "src_null", "tgt_null", "results_null", "index_high", "index_negative",
                                  "sharing_high", "sharing_negative", "k_lrf_zero"])
def test_invalid_arguments(mod, case):
    from se3icp import _lib
    kw = {
        "n_clouds_zero": dict(n_clouds=0), "n_clouds_negative": dict(n_clouds=-2),
        "n_pairs_zero": dict(n_pairs=0), "n_pairs_negative": dict(n_pairs=-1),
        "xyz_null": dict(null="xyz"), "n_pts_null": dict(null="n_pts"), "src_null": dict(null="src"),
        "tgt_null": dict(null="tgt"), "results_null": dict(null="results"),
        "index_high": dict(src=(1, 3)), "index_negative": dict(tgt=(0, -1)),
        "sharing_high": dict(sharing=4), "sharing_negative": dict(sharing=-1),
        "k_lrf_zero": dict(params=_lib.default_params(number_of_nn_for_LRF=0)),
    }[case]
    assert _call(**kw) == _lib.ERR_INVALID_ARG


def test_valid_shapes_reach_the_device_lookup(mod):
    """A self edge, a repeated edge, an unused (even empty) cloud, any order, every sharing
    level, every method, default parameters (NULL)."""
    from se3icp import _lib
    assert _call(src=(1, 1, 2, 1), tgt=(1, 0, 0, 0)) == _lib.ERR_NO_DEVICE
    assert _call(n_pts=(50, 0, 70), src=(2,), tgt=(0,)) == _lib.ERR_NO_DEVICE
    assert _call(params=None) == _lib.ERR_NO_DEVICE
    for lv in (0, 1, 2, 3):
        assert _call(sharing=lv) == _lib.ERR_NO_DEVICE
    for m in _lib.METHODS:
        assert _call(method=m) == _lib.ERR_NO_DEVICE, m


def test_empty_cloud_that_an_edge_uses(mod):
    from se3icp import _lib
    assert _call(n_pts=(50, 0, 70)) == _lib.ERR_EMPTY_CLOUD
    assert _call(n_pts=(0, 60, 70), src=(1,), tgt=(0,)) == _lib.ERR_EMPTY_CLOUD


def test_unknown_method(mod):
    from se3icp import _lib
    assert _call(method=10) == _lib.ERR_INVALID_METHOD
    assert _call(method=-3) == _lib.ERR_INVALID_METHOD


def test_device_and_report_entries_check_before_the_device(mod):
    from se3icp import _lib
    L = _lib.load()
    res = (_lib.Result * 2)()
    rep = (_lib.Report * 2)()
    off = (C.c_int64 * 4)(0, 10, 30, 35)
    empty = (C.c_int64 * 4)(0, 10, 10, 35)
    es, et = (C.c_int32 * 2)(1, 2), (C.c_int32 * 2)(0, 1)
    bad = (C.c_int32 * 2)(1, 3)
    ptr = C.c_void_p(4096)  # never dereferenced: no device is reached
    opts = _lib.ReportOptions(0.0, None, None, 0, 0)
    nan = _lib.ReportOptions(float("nan"), None, None, 0, 0)

    def call(o=off, s=es, method=5, sharing=0, xyz=ptr, nc=3):
        return L.se3icp_register_graph_device(NO_SUCH_DEVICE, nc, xyz, o, 2, s, et, method, None, sharing, res, None)

    assert call() == _lib.ERR_NO_DEVICE
    assert call(xyz=None) == _lib.ERR_INVALID_ARG
    assert call(o=None) == _lib.ERR_INVALID_ARG
    assert call(nc=0) == _lib.ERR_INVALID_ARG
    assert call(s=bad) == _lib.ERR_INVALID_ARG
    assert call(sharing=7) == _lib.ERR_INVALID_ARG
    assert call(o=empty) == _lib.ERR_EMPTY_CLOUD
    assert call(method=99) == _lib.ERR_INVALID_METHOD

    def rcall(o=opts, r=rep, sharing=0):
        return L.se3icp_register_graph_report_device(NO_SUCH_DEVICE, 3, ptr, off, 2, es, et, 5, None, sharing, res, None,
                                                     C.byref(o) if o is not None else None, r)

    assert rcall() == _lib.ERR_NO_DEVICE
    assert rcall(o=None) == _lib.ERR_INVALID_ARG
    assert rcall(r=None) == _lib.ERR_INVALID_ARG
    assert rcall(o=nan) == _lib.ERR_INVALID_ARG
    assert rcall(sharing=-1) == _lib.ERR_INVALID_ARG
    out = (C.c_int64 * 9)()
    assert L.se3icp_last_graph_stats(NO_SUCH_DEVICE, out, 8) == _lib.ERR_INVALID_ARG
    assert L.se3icp_last_graph_stats(NO_SUCH_DEVICE, None, 9) == _lib.ERR_INVALID_ARG
    assert L.se3icp_last_graph_stats(NO_SUCH_DEVICE, out, 9) == _lib.ERR_NO_DEVICE


def test_sequence_edges(mod):
    assert mod.sequence_edges(0) == [] and mod.sequence_edges(1) == []
    assert mod.sequence_edges(2) == [(1, 0)]
    assert mod.sequence_edges(5) == [(1, 0), (2, 1), (3, 2), (4, 3)]
    clouds = [np.full((2, 3), float(i)) for i in range(4)]
    pairs = mod.expand_edges(clouds, mod.sequence_edges(4) + [(2, 2)])
    assert [(int(s[0, 0]), int(t[0, 0])) for s, t in pairs] == [(1, 0), (2, 1), (3, 2), (2, 2)]
    assert pairs[1][0] is clouds[2] and pairs[3][1] is clouds[2]


def test_header_symbols_are_exported(mod):
    from se3icp import _lib
    L = _lib.load()
    for name in ("se3icp_register_graph", "se3icp_register_graph_device", "se3icp_register_graph_report",
                 "se3icp_register_graph_report_device", "se3icp_last_graph_stats"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    assert len(_lib.GRAPH_STATS) == 9
    assert L.se3icp_abi_version() == 4  # only new functions: the ABI version stays


@pytest.fixture(scope="module")
def plan_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("gr") / "graph_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "graph_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}


@pytest.mark.parametrize("check", ["scale", "equal", "self", "repeat", "unused", "order", "level1", "vanilla", "cover",
                                   "args"])
def test_class_planning(plan_report, check):
    rc, report = plan_report
    assert report.get(check) == check + " ok", report.get(check)


def test_class_planning_program(plan_report):
    rc, report = plan_report
    assert rc == 0, report
    assert int(report["checked"].split()[1]) > 1000
