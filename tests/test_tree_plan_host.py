"""CPU tests of the host side of one kd-tree order per cloud: the argument checks of
se3icp_set_tree_sharing and se3icp_last_tree_stats (they run before the device is looked up, so a
bad call is reported as such on a host without a GPU), the loud failure without a device, and the
tree plan of se3-icp_amd/csrc/graph.hpp (graph_plan_trees) built for the host
(tests/tree_plan_host.cpp), plain and under AddressSanitizer + UndefinedBehaviorSanitizer, as
test_seed_host.py builds the seed plan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "se3-icp_amd", "csrc")
NO_SUCH_DEVICE = 200  # an ordinal no machine has: the calls below never reach a GPU
CHECKS = ["chain", "map", "unconfirmed", "level1", "vanilla", "random"]


@pytest.fixture(scope="module")
def mod():
    import se3icp
    se3icp.load()
    return se3icp


@pytest.mark.parametrize("mode", [-1, 2, 3, 100, -(2 ** 31)])
def test_invalid_mode(mod, mode):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_tree_sharing(NO_SUCH_DEVICE, mode) == _lib.ERR_INVALID_ARG
    assert L.se3icp_set_tree_sharing(0, mode) == _lib.ERR_INVALID_ARG  # whether or not device 0 exists
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_tree_sharing(mode, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("mode", [0, 1])
def test_valid_mode_without_device_fails_loudly(mod, mode):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_tree_sharing(NO_SUCH_DEVICE, mode) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_tree_sharing(-1, mode) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_tree_sharing(0 | 16 << 8, mode) == _lib.ERR_NO_DEVICE  # engine slots end at 15
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_tree_sharing(mode, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    if mod.device_count() == 0:  # and on the default device of a host without one
        with pytest.raises(mod.Se3IcpError) as e:
            mod.set_tree_sharing(mode)
        assert e.value.code == _lib.ERR_NO_DEVICE


def test_tree_stats_arguments(mod):
    from se3icp import _lib
    L = _lib.load()
    out = (C.c_int64 * 4)()
    for device in (NO_SUCH_DEVICE, 0):
        assert L.se3icp_last_tree_stats(device, None, 4) == _lib.ERR_INVALID_ARG
        assert L.se3icp_last_tree_stats(device, out, 3) == _lib.ERR_INVALID_ARG
        assert L.se3icp_last_tree_stats(device, out, -1) == _lib.ERR_INVALID_ARG
    assert L.se3icp_last_tree_stats(NO_SUCH_DEVICE, out, 4) == _lib.ERR_NO_DEVICE
    assert L.se3icp_last_tree_stats(NO_SUCH_DEVICE, out, 9) == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.last_tree_stats(device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    assert _lib.TREE_STATS == ["built_3d", "adopted_3d", "built_12d", "adopted_12d"]


def test_header_symbols_are_exported(mod):
    from se3icp import _lib
    L = _lib.load()
    for sym in ("se3icp_set_tree_sharing", "se3icp_last_tree_stats"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "set_tree_sharing" in mod.__all__ and "last_tree_stats" in mod.__all__
    assert L.se3icp_abi_version() == 4  # only new functions: the ABI version stays
    with open(os.path.join(ROOT, "include", "se3icp.h")) as f:
        text = f.read()
    assert "int se3icp_set_tree_sharing(int device, int mode);" in text
    assert "int se3icp_last_tree_stats(int device, int64_t* out, int n);" in text
    assert "#define SE3ICP_TREE_STATS_N 4" in text


def _build_and_run(tmp_path_factory, name, flags):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp(name) / "tree_plan_host")
    subprocess.check_call([cc, "-std=c++17", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tree_plan_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}, out.stderr


@pytest.fixture(scope="module")
def plan_report(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "tp", ["-O2"])


@pytest.fixture(scope="module")
def plan_report_sanitized(tmp_path_factory):
    """The same stand-alone program, host code only, under ASan + UBSan (any finding aborts)."""
    return _build_and_run(tmp_path_factory, "tps", ["-O1", "-g", "-fsanitize=address,undefined",
                                                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("check", CHECKS)
def test_tree_plan(plan_report, check):
    rc, report, _ = plan_report
    assert report.get(check) == check + " ok", report.get(check)


def test_tree_plan_program(plan_report):
    rc, report, err = plan_report
    assert rc == 0, (report, err)
    assert int(report["checked"].split()[1]) > 1000


def test_tree_plan_program_sanitized(plan_report_sanitized):
    rc, report, err = plan_report_sanitized
    assert rc == 0 and err == "", (report, err)
    for check in CHECKS:
        assert report.get(check) == check + " ok", report.get(check)
