"""CPU tests of the host side of taking a source class's neighbour lists: the
argument checks of se3icp_set_lrf_taking and se3icp_last_take_stats (they run before the device
is looked up), the loud failure without a device, and tests/take_host.cpp, a stand-alone program
that checks the plan (graph_plan_takes), narrow_bound against widen_bound, and the certificate's
bound against long double evaluation -- built and run a second time under ASan + UBSan."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "se3-icp_amd", "csrc")
NO_SUCH_DEVICE = 200  # an ordinal no machine has: the calls below never reach a GPU
CHECKS = ["chain", "map", "kw", "centre", "posed", "treeoff", "level1", "random", "narrow", "certificate"]


@pytest.fixture(scope="module")
def mod():
    import se3icp
    se3icp.load()
    return se3icp


@pytest.mark.parametrize("mode", [-1, 3, 4, 100, -(2 ** 31)])
def test_invalid_mode(mod, mode):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_lrf_taking(NO_SUCH_DEVICE, mode) == _lib.ERR_INVALID_ARG
    assert L.se3icp_set_lrf_taking(0, mode) == _lib.ERR_INVALID_ARG  # whether or not device 0 exists
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_lrf_taking(mode, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_valid_mode_without_device_fails_loudly(mod, mode):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_lrf_taking(NO_SUCH_DEVICE, mode) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_lrf_taking(-1, mode) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_lrf_taking(0 | 16 << 8, mode) == _lib.ERR_NO_DEVICE  # engine slots end at 15
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_lrf_taking(mode, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE


def test_take_stats_arguments(mod):
    from se3icp import _lib
    L = _lib.load()
    out = (C.c_int64 * 4)()
    for device in (NO_SUCH_DEVICE, 0):
        assert L.se3icp_last_take_stats(device, None, 4) == _lib.ERR_INVALID_ARG
        assert L.se3icp_last_take_stats(device, out, 3) == _lib.ERR_INVALID_ARG
        assert L.se3icp_last_take_stats(device, out, -1) == _lib.ERR_INVALID_ARG
    assert L.se3icp_last_take_stats(NO_SUCH_DEVICE, out, 4) == _lib.ERR_NO_DEVICE
    assert L.se3icp_last_take_stats(NO_SUCH_DEVICE, out, 9) == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.last_take_stats(device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    assert _lib.TAKE_STATS == ["classes_taking", "queries_taken", "queries_redone", "queries_failed"]


def test_header_symbols_are_exported(mod):
    from se3icp import _lib
    L = _lib.load()
    for sym in ("se3icp_set_lrf_taking", "se3icp_last_take_stats"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "set_lrf_taking" in mod.__all__ and "last_take_stats" in mod.__all__
    assert L.se3icp_abi_version() == 4  # only new functions: the ABI version stays
    with open(os.path.join(ROOT, "include", "se3icp.h")) as f:
        text = f.read()
    assert "int se3icp_set_lrf_taking(int device, int mode);" in text
    assert "int se3icp_last_take_stats(int device, int64_t* out, int n);" in text
    assert "#define SE3ICP_TAKE_STATS_N 4" in text


def _build_and_run(tmp_path_factory, name, flags):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp(name) / "take_host")
    subprocess.check_call([cc, "-std=c++17", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "take_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}, out.stderr


@pytest.fixture(scope="module")
def take_report(tmp_path_factory):
    return _build_and_run(tmp_path_factory, "tk", ["-O2"])


@pytest.fixture(scope="module")
def take_report_sanitized(tmp_path_factory):
    """The same stand-alone program, host code only, under ASan + UBSan (any finding aborts)."""
    return _build_and_run(tmp_path_factory, "tks", ["-O1", "-g", "-fsanitize=address,undefined",
                                                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])


@pytest.mark.parametrize("check", CHECKS)
def test_take_host(take_report, check):
    rc, report, _ = take_report
    assert report.get(check) == check + " ok", (report.get(check), report.get("FAILED"))


def test_take_host_program(take_report):
    rc, report, err = take_report
    assert rc == 0, (report, err)
    assert int(report["checked"].split()[1]) > 100000


def test_take_host_program_sanitized(take_report_sanitized):
    rc, report, err = take_report_sanitized
    assert rc == 0 and err == "", (report, err)
    for check in CHECKS:
        assert report.get(check) == check + " ok", report.get(check)
