"""CPU tests of the host side of content-detected sharing in the device batch entries: the
argument checks of se3icp_set_batch_sharing (they run before the device is looked up, so a bad
level is reported as such on a host without a GPU), the loud failure without a device, and the
slot grouping of se3-icp_amd/csrc/graph.hpp -- candidates by (point count, hash), the compare's
confirm flags, hash-equal but unconfirmed slots, the per-use class plan -- built for the host
(tests/share_host.cpp) as test_graph_host.py builds the class planning."""
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


@pytest.mark.parametrize("level", [-1, 3, 4, 100, -(2 ** 31)])
def test_invalid_level(mod, level):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_batch_sharing(NO_SUCH_DEVICE, level) == _lib.ERR_INVALID_ARG
    assert L.se3icp_set_batch_sharing(0, level) == _lib.ERR_INVALID_ARG  # whether or not device 0 exists
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_batch_sharing(level, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("level", [0, 1, 2])
def test_valid_level_without_device_fails_loudly(mod, level):
    from se3icp import _lib
    L = _lib.load()
    assert L.se3icp_set_batch_sharing(NO_SUCH_DEVICE, level) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_batch_sharing(-1, level) == _lib.ERR_NO_DEVICE
    assert L.se3icp_set_batch_sharing(0 | 16 << 8, level) == _lib.ERR_NO_DEVICE  # engine slots end at 15
    with pytest.raises(mod.Se3IcpError) as e:
        mod.set_batch_sharing(level, device=NO_SUCH_DEVICE)
    assert e.value.code == _lib.ERR_NO_DEVICE
    if mod.device_count() == 0:  # and on the default device of a host without one
        with pytest.raises(mod.Se3IcpError) as e:
            mod.set_batch_sharing(level)
        assert e.value.code == _lib.ERR_NO_DEVICE


def test_header_symbol_is_exported(mod):
    from se3icp import _lib
    L = _lib.load()
    assert "se3icp_set_batch_sharing" in _lib.EXPORTED_SYMBOLS and hasattr(L, "se3icp_set_batch_sharing")
    assert "set_batch_sharing" in mod.__all__
    assert L.se3icp_abi_version() == 4  # only a new function: the ABI version stays
    with open(os.path.join(ROOT, "include", "se3icp.h")) as f:
        assert "int se3icp_set_batch_sharing(int device, int level);" in f.read()


@pytest.fixture(scope="module")
def share_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("sh") / "share_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "share_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}


@pytest.mark.parametrize("check", ["equal_n", "group", "confirm", "chain", "random", "uses"])
def test_slot_grouping(share_report, check):
    rc, report = share_report
    assert report.get(check) == check + " ok", report.get(check)


def test_slot_grouping_program(share_report):
    rc, report = share_report
    assert rc == 0, report
    assert int(report["checked"].split()[1]) > 1000
