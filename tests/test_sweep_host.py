"""CPU tests of the parameter sweep's host side: the argument checks of
se3icp_register_sweep(_device) (they run before the device is looked up, so a bad call is
reported as such on a host without a GPU), the loud failure without a device, the
reference's alpha grid, and the group rule of se3-icp_amd/csrc/sweep.hpp, built for the
host (tests/sweep_group_host.cpp) as test_tree_layout.py builds tree.hpp."""
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


def _call(mod, n_src=(50,), n_tgt=(60,), method="se3_gicp", variants="default", max_group=0, n_variants=None,
          device=NO_SUCH_DEVICE):
    """se3icp_register_sweep with one knob turned; returns the status."""
    from se3icp import _lib
    L = _lib.load()
    n = len(n_src)
    dp = C.POINTER(C.c_double)
    rng = np.random.default_rng(0)
    srcs = [rng.random((max(k, 1), 3)) for k in n_src]
    tgts = [rng.random((max(k, 1), 3)) for k in n_tgt]
    sp = (dp * n)(*[a.ctypes.data_as(dp) for a in srcs])
    tp = (dp * n)(*[a.ctypes.data_as(dp) for a in tgts])
    ns = (C.c_int64 * n)(*n_src)
    nt = (C.c_int64 * n)(*n_tgt)
    if variants == "default":
        variants = [mod.default_params(alpha_rot=a) for a in (0.5, 3.0)]
    nv = len(variants) if variants is not None else 2
    arr = None
    if variants:
        arr = (_lib.Params * len(variants))()
        for i, p in enumerate(variants):
            C.memmove(C.byref(arr, i * C.sizeof(_lib.Params)), C.byref(p), C.sizeof(_lib.Params))
    res = (_lib.Result * max(1, nv * n))()
    mid = method if isinstance(method, int) else _lib.method_id(method)
    return L.se3icp_register_sweep(device, n, sp, ns, tp, nt, mid, nv if n_variants is None else n_variants, arr,
                                   max_group, res)


def test_valid_call_without_device_fails_loudly(mod):
    from se3icp import _lib
    assert _call(mod) == _lib.ERR_NO_DEVICE
    a = np.random.default_rng(1).random((40, 3))
    variants = mod.sweep_params(mod.default_params(), alpha_rot=[1.0, 2.0])
    with pytest.raises(mod.Se3IcpError) as e:
        mod.register_sweep([(a, a)], "se3_pt2pl", variants, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    if mod.device_count() == 0:  # and on the default device of a host without one
        with pytest.raises(mod.Se3IcpError) as e:
            mod.register_sweep([(a, a)], "se3_pt2pl", variants)
        assert e.value.code == _lib.ERR_NO_DEVICE


@pytest.mark.parametrize("case", ["n_variants_zero", "n_variants_negative", "variants_null", "max_group_negative",
                                  "k_lrf_differs", "scale_differs"])
def test_invalid_arguments(mod, case):
    from se3icp import _lib
    kw = {}
    if case == "n_variants_zero":
        kw = dict(n_variants=0)
    elif case == "n_variants_negative":
        kw = dict(n_variants=-1)
    elif case == "variants_null":
        kw = dict(variants=None)
    elif case == "max_group_negative":
        kw = dict(max_group=-1)
    elif case == "k_lrf_differs":
        kw = dict(variants=[mod.default_params(number_of_nn_for_LRF=30), mod.default_params(number_of_nn_for_LRF=31)])
    elif case == "scale_differs":
        kw = dict(variants=[mod.default_params(scale_preprocessing=3.0), mod.default_params(scale_preprocessing=1.5)])
    assert _call(mod, **kw) == _lib.ERR_INVALID_ARG


def test_every_other_field_may_differ(mod):
    """... so such variants pass the checks and reach the device lookup."""
    from se3icp import _lib
    variants = [mod.default_params(alpha_rot=0.0, beta_transl=0.25, estimated_overlap=0.05, max_num_iterations=11,
                                   max_num_se3_iterations=1, mse=1e-7, mse_switch_error=5e-4),
                mod.default_params()]
    assert _call(mod, variants=variants, max_group=7) == _lib.ERR_NO_DEVICE
    for m in _lib.METHODS:  # all ten methods are accepted
        assert _call(mod, method=m) == _lib.ERR_NO_DEVICE, m


def test_empty_clouds(mod):
    from se3icp import _lib
    assert _call(mod, n_src=(50, 0), n_tgt=(60, 10)) == _lib.ERR_EMPTY_CLOUD
    assert _call(mod, n_src=(50,), n_tgt=(0,)) == _lib.ERR_EMPTY_CLOUD


def test_unknown_method(mod):
    from se3icp import _lib
    assert _call(mod, method=10) == _lib.ERR_INVALID_METHOD
    assert _call(mod, method=-3) == _lib.ERR_INVALID_METHOD


def test_device_entry_checks_before_the_device(mod):
    from se3icp import _lib
    L = _lib.load()
    res = (_lib.Result * 4)()
    off = (C.c_int64 * 2)(0, 10)
    empty = (C.c_int64 * 2)(5, 5)
    arr = (_lib.Params * 2)(mod.default_params(), mod.default_params())
    ptr = C.c_void_p(4096)  # never dereferenced: no device is reached

    def call(so=off, to=off, nv=2, v=arr, mg=0, method=5):
        return L.se3icp_register_sweep_device(NO_SUCH_DEVICE, 1, ptr, so, ptr, to, method, nv, v, mg, res, None)

    assert call() == _lib.ERR_NO_DEVICE
    assert call(nv=0) == _lib.ERR_INVALID_ARG
    assert call(v=None) == _lib.ERR_INVALID_ARG
    assert call(mg=-2) == _lib.ERR_INVALID_ARG
    assert call(so=empty) == _lib.ERR_EMPTY_CLOUD
    assert call(method=99) == _lib.ERR_INVALID_METHOD


def test_alpha_grid(mod):
    g = mod.alpha_grid()
    assert len(g) == 47
    assert g == sorted(g) and len(set(g)) == 47
    assert g[0] == 0.0 and g[-1] == 1000.0
    assert 3 * 0.1 in g and 0.3 not in g  # the reference's i * 0.1, not the literal
    assert 1.0 in g and 5.0 in g and g.count(1.0) == 1


def test_sweep_params(mod):
    base = mod.kitti_params()
    v = mod.sweep_params(base, alpha_rot=[0.5, 2.0, 9.0], beta_transl=[1.0, 2.0, 3.0])
    assert [(p.alpha_rot, p.beta_transl) for p in v] == [(0.5, 1.0), (2.0, 2.0), (9.0, 3.0)]
    assert all(p.mse == base.mse and p.number_of_nn_for_LRF == 90 for p in v)
    assert base.alpha_rot == 3.0  # the base is copied, not written
    with pytest.raises(ValueError):
        mod.sweep_params(base, alpha_rot=[1.0], beta_transl=[1.0, 2.0])
    with pytest.raises(ValueError):
        mod.sweep_params(base, no_such_field=[1.0])


@pytest.fixture(scope="module")
def group_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("sw") / "sweep_group_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "sweep_group_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}


@pytest.mark.parametrize("check", ["range", "bound", "points", "budget", "cover", "fill"])
def test_group_rule(group_report, check):
    rc, report = group_report
    assert report.get(check) == check + " ok", report.get(check)


def test_group_rule_program(group_report):
    rc, report = group_report
    assert rc == 0, report
    assert int(report["checked"].split()[1]) == 50 * 12 * 13 * 3 * 5
