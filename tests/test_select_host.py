"""CPU tests of the neighbour selection's plan (se3-icp_amd/csrc/graph.hpp: graph_plan_selection,
what Engine::select_by_class decides before it queues anything, and select_wave_tables, the wave
tables of Engine::setup_knn): tests/select_host.cpp, a stand-alone program that checks what the
kernels rely on over the chain, the map, a posed graph and random graphs -- built and run a second
time under ASan + UBSan, and once per planted defect, which must make it fail."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "se3-icp_amd", "csrc")
CHECKS = ["home", "seg", "chunks", "stores", "loads", "take", "stride", "off", "waves", "expected"]
PLANTED = {"overlap": "stores", "early": "loads", "orphan": "take", "twice": "waves"}


def _build(tmp_path_factory, name, flags):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp(name) / "select_host")
    subprocess.check_call([cc, "-std=c++17", *flags, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "select_host.cpp"), "-o", exe])
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}, out.stderr


@pytest.fixture(scope="module")
def select_exe(tmp_path_factory):
    return _build(tmp_path_factory, "sl", ["-O2"])


@pytest.fixture(scope="module")
def select_report(select_exe):
    return _run(select_exe)


@pytest.fixture(scope="module")
def select_report_sanitized(tmp_path_factory):
    """The same stand-alone program, host code only, under ASan + UBSan (any finding aborts)."""
    return _run(_build(tmp_path_factory, "sls", ["-O1", "-g", "-fsanitize=address,undefined",
                                                 "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]))


@pytest.mark.parametrize("check", CHECKS + ["planted_" + p for p in PLANTED])
def test_select_host(select_report, check):
    rc, report, _ = select_report
    assert report.get(check) == check + " ok", report.get(check)


def test_select_host_program(select_report):
    rc, report, err = select_report
    assert rc == 0, (report, err)
    assert int(report["checked"].split()[1]) > 100000


def test_select_host_program_sanitized(select_report_sanitized):
    rc, report, err = select_report_sanitized
    assert rc == 0 and err == "", (report, err)
    for check in CHECKS + ["planted_" + p for p in PLANTED]:
        assert report.get(check) == check + " ok", report.get(check)


@pytest.mark.parametrize("defect", sorted(PLANTED))
def test_planted_defect_fails_the_program(select_exe, defect):
    """With the defect planted in every plan before it is checked, the program reports the check
    that guards it and exits 1."""
    rc, report, err = _run(select_exe, "--plant", defect)
    assert rc == 1, (report, err)
    assert report[PLANTED[defect]].startswith(PLANTED[defect] + " FAIL"), report


def test_unknown_defect_is_an_error(select_exe):
    assert _run(select_exe, "--plant", "nothing")[0] == 2
