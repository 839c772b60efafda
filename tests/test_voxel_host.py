"""CPU tests of the voxel-grid downsample's host side: the key arithmetic of
se3-icp_amd/csrc/voxel.hpp built for the host (tests/voxel_host.cpp: packing round trips at the
axis bit lengths (1,1,1), (21,21,21), (31,31,1), (62,1,0) and more, the 63-bit rule, Open3D's
"voxel_size is too small" at its edge, the cell arithmetic), and through ctypes every argument
error of the two entries with its status -- they are checked before the device is looked up, so
a bad call is reported as such on a host without a GPU -- and the loud failure without a device."""
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
DP, IP, LP = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def mod():
    import se3icp
    se3icp.load()
    return se3icp


@pytest.fixture(scope="module")
def voxel_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("vx") / "voxel_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "voxel_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}


@pytest.mark.parametrize("check", ["pack", "overflow", "too_small", "cells", "sizes"])
def test_key_arithmetic(voxel_report, check):
    rc, report = voxel_report
    assert report.get(check) == check + " ok", report.get(check)


def test_key_arithmetic_program(voxel_report):
    rc, report = voxel_report
    assert rc == 0, report
    assert int(report["checked"].split()[1]) > 10000


def _host(L, device, xyz, n, v):
    return L.se3icp_voxel_downsample(device, xyz.ctypes.data_as(DP) if xyz is not None else None, n, v, None, None, None)


def _device(L, device, nc, xyz_ptr, off, vs, out_ptr, out_off=True):
    o = (C.c_int64 * len(off))(*off) if off is not None else None
    v = (C.c_double * max(1, len(vs)))(*vs) if vs is not None else None
    oo = (C.c_int64 * (max(nc, 0) + 1))() if out_off else None
    return L.se3icp_voxel_downsample_device(device, nc, C.c_void_p(xyz_ptr), o, v, C.c_void_p(out_ptr), oo, None, None,
                                            None)


@pytest.mark.parametrize("device", [0, NO_SUCH_DEVICE, 1 << 8])
def test_argument_errors_before_the_device(mod, device):
    from se3icp import _lib
    L = _lib.load()
    xyz = np.random.default_rng(0).random((10, 3))
    for v in (0.0, -0.1, float("nan"), float("inf"), -float("inf")):
        assert _host(L, device, xyz, 10, v) == _lib.ERR_INVALID_ARG, v
        assert _device(L, device, 2, 4096, [0, 5, 10], [0.1, v], 8192) == _lib.ERR_INVALID_ARG, v
    assert _host(L, device, xyz, 0, 0.1) == _lib.ERR_EMPTY_CLOUD
    assert _host(L, device, xyz, -1, 0.1) == _lib.ERR_INVALID_ARG
    assert _host(L, device, None, 10, 0.1) == _lib.ERR_INVALID_ARG
    assert _device(L, device, 3, 4096, [0, 5, 5, 10], [0.1, 0.1, 0.1], 8192) == _lib.ERR_EMPTY_CLOUD
    assert _device(L, device, 2, 4096, [0, 5, 3], [0.1, 0.1], 8192) == _lib.ERR_INVALID_ARG  # offsets go back
    assert _device(L, device, 0, 4096, [0], [0.1], 8192) == _lib.ERR_INVALID_ARG
    assert _device(L, device, -1, 4096, [0], [0.1], 8192) == _lib.ERR_INVALID_ARG
    assert _device(L, device, 1, 4096, None, [0.1], 8192) == _lib.ERR_INVALID_ARG
    assert _device(L, device, 1, 4096, [0, 5], None, 8192) == _lib.ERR_INVALID_ARG
    assert _device(L, device, 1, 0, [0, 5], [0.1], 8192) == _lib.ERR_INVALID_ARG       # no input
    assert _device(L, device, 1, 4096, [0, 5], [0.1], 0) == _lib.ERR_INVALID_ARG       # no output
    assert _device(L, device, 1, 4096, [0, 5], [0.1], 8192, out_off=False) == _lib.ERR_INVALID_ARG


def test_python_wrappers_raise_the_status(mod):
    from se3icp import _lib
    xyz = np.random.default_rng(1).random((10, 3))
    for v, code in ((0.0, _lib.ERR_INVALID_ARG), (float("nan"), _lib.ERR_INVALID_ARG)):
        with pytest.raises(mod.Se3IcpError) as e:
            mod.voxel_downsample(xyz, v, device=NO_SUCH_DEVICE)
        assert e.value.code == code
        with pytest.raises(mod.Se3IcpError) as e:
            mod.voxel_downsample_device(4096, [0, 10], v, 8192, device=NO_SUCH_DEVICE)
        assert e.value.code == code
    with pytest.raises(mod.Se3IcpError) as e:
        mod.voxel_downsample(np.zeros((0, 3)), 0.1, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_EMPTY_CLOUD
    with pytest.raises(mod.Se3IcpError) as e:
        mod.voxel_downsample_device(4096, [0, 10, 10], [0.1, 0.2], 8192, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_EMPTY_CLOUD


def test_valid_call_without_device_fails_loudly(mod):
    from se3icp import _lib
    L = _lib.load()
    xyz = np.random.default_rng(2).random((10, 3))
    for device in (NO_SUCH_DEVICE, -1, 0 | 16 << 8):  # engine slots end at 15
        assert _host(L, device, xyz, 10, 0.1) == _lib.ERR_NO_DEVICE
        assert _device(L, device, 1, 4096, [0, 10], [0.1], 8192) == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.voxel_downsample(xyz, 0.1, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    if mod.device_count() == 0:  # and on the default device of a host without one: never a CPU result
        assert _host(L, 0, xyz, 10, 0.1) == _lib.ERR_NO_DEVICE
        assert _device(L, 0, 1, 4096, [0, 10], [0.1], 8192) == _lib.ERR_NO_DEVICE
        with pytest.raises(mod.Se3IcpError) as e:
            mod.voxel_downsample(xyz, 0.1)
        assert e.value.code == _lib.ERR_NO_DEVICE
        with pytest.raises(mod.Se3IcpError) as e:
            mod.voxel_downsample_device(4096, [0, 10], 0.1, 8192)
        assert e.value.code == _lib.ERR_NO_DEVICE


def test_header_symbols_are_exported(mod):
    from se3icp import _lib
    L = _lib.load()
    for sym in ("se3icp_voxel_version", "se3icp_voxel_downsample_device", "se3icp_voxel_downsample"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "voxel_downsample" in mod.__all__ and "voxel_downsample_device" in mod.__all__
    assert L.se3icp_voxel_version() == 1
    assert L.se3icp_abi_version() == 4  # only new functions: the ABI version stays
    with open(os.path.join(ROOT, "include", "se3icp.h")) as f:
        h = f.read()
    assert "int se3icp_voxel_downsample_device(int device, int32_t n_clouds, const double* d_xyz" in h
    assert "int64_t se3icp_voxel_downsample(int device, const double* xyz, int64_t n, double voxel_size" in h
    assert "DEPARTURE FROM OPEN3D" in h  # the 63-bit rule is stated


def test_keywords_default_to_the_old_path(mod):
    import inspect
    for f in (mod.register_graph, mod.register_sequence):
        assert inspect.signature(f).parameters["voxel_size"].default is None
