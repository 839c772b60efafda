"""CPU tests of the host side of seeding a cloud's later classes from its first class's neighbour
distances: the argument checks of se3icp_set_lrf_seeding and se3icp_last_seed_stats (they run
before the device is looked up, so a bad call is reported as such on a host without a GPU), the
loud failure without a device, and the seed plan of se3-icp_amd/csrc/graph.hpp
(graph_plan_seeds) built for the host (tests/seed_host.cpp) as test_share_host.py builds the
slot grouping."""
import ctypes as C
import os
import shutil
import subprocess

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


@pytest.mark.parametrize("mode", [-1, 4, 5, 100, -(2 ** 31)])
def test_invalid_mode(mod, mode):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_lrf_seeding(NO_SUCH_DEVICE, mode) == _lib.ERR_INVALID_ARG
    assert L.se3icp_set_lrf_seeding(0, mode) == _lib.ERR_INVALID_ARG  # whether or not device 0 exists
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_lrf_seeding(mode, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_valid_mode_without_device_fails_loudly(mod, mode):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_lrf_seeding(NO_SUCH_DEVICE, mode) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_lrf_seeding(-1, mode) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_lrf_seeding(0 | 16 << 8, mode) == _lib.ERR_NO_DEVICE  # engine slots end at 15
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_lrf_seeding(mode, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    if mod.device_count() == 0:  # and on the default device of a host without one
        with pytest.raises(mod.Se3IcpError) as e:
            mod.set_lrf_seeding(mode)
        assert e.value.code == _lib.ERR_NO_DEVICE


def test_seed_stats_arguments(mod):
    from se3icp import _lib
    L = _lib.load()
    out = (C.c_int64 * 4)()
    for device in (NO_SUCH_DEVICE, 0):
        assert L.se3icp_last_seed_stats(device, None, 4) == _lib.ERR_INVALID_ARG
        assert L.se3icp_last_seed_stats(device, out, 3) == _lib.ERR_INVALID_ARG
        assert L.se3icp_last_seed_stats(device, out, -1) == _lib.ERR_INVALID_ARG
    assert L.se3icp_last_seed_stats(NO_SUCH_DEVICE, out, 4) == _lib.ERR_NO_DEVICE
    assert L.se3icp_last_seed_stats(NO_SUCH_DEVICE, out, 9) == _lib.ERR_NO_DEVICE
    with pytest.raises(mod.Se3IcpError) as e:
        mod.last_seed_stats(device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    assert len(_lib.SEED_STATS) == 4


def test_header_symbols_are_exported(mod):
    from se3icp import _lib
    L = _lib.load()
    for sym in ("se3icp_set_lrf_seeding", "se3icp_last_seed_stats"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert "set_lrf_seeding" in mod.__all__ and "last_seed_stats" in mod.__all__
    assert L.se3icp_abi_version() == 4  # only new functions: the ABI version stays
    with open(os.path.join(ROOT, "include", "se3icp.h")) as f:
        text = f.read()
    assert "int se3icp_set_lrf_seeding(int device, int mode);" in text
    assert "int se3icp_last_seed_stats(int device, int64_t* out, int n);" in text
    assert "#define SE3ICP_SEED_STATS_N 4" in text


@pytest.fixture(scope="module")
def seed_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("sd") / "seed_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "seed_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}


@pytest.mark.parametrize("check", ["chain", "map", "kw", "vanilla", "level1", "random"])
def test_seed_plan(seed_report, check):
    rc, report = seed_report
    assert report.get(check) == check + " ok", report.get(check)


def test_seed_plan_program(seed_report):
    rc, report = seed_report
    assert rc == 0, report
    assert int(report["checked"].split()[1]) > 1000
