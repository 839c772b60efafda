"""CPU test of the kd-tree layout arithmetic in se3-icp_amd/csrc/tree.hpp: the helpers are
__host__ __device__, so the source the kernels use is built here for the host
(tests/tree_layout_host.cpp) and checked for every single-cloud size n in 1 .. 300,000, a
handful of sizes around 2^k * 4096 up to 2^22, and every level (the checks are listed in
the program's header).

The defect this pins: k_tree_local chose between its wave sort (sub-nodes of <= 512 points)
and its LDS partition (laid out for <= 4 sub-nodes) from the estimate ceil(m / nsub) + 1,
which reads 513 for a level-G node of m = 4089 .. 4096 points at nsub = 8.  Eight sub-nodes
then went through the partition, whose histogram clear ran over the node's permutation.
Clouds with ceil(n / 2^G) in 4089 .. 4096 were hit: n in 4089-4096, 8177-8192, 16353-16384,
32705-32768, 65409-65536, 130817-131072, 261633-262144 (1,016 of the first 300,000 sizes);
built against that estimate, this program reports exactly those sizes under `partition`.
tree_local_sort_per now decides from tree_max_node, the exact bound."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(ROOT, "se3-icp_amd", "csrc")


@pytest.fixture(scope="module")
def layout_report(tmp_path_factory):
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not cc:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("tl") / "tree_layout_host")
    subprocess.check_call([cc, "-std=c++17", "-O2", "-pthread", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tree_layout_host.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    return out.returncode, {ln.split()[0]: ln for ln in lines}


@pytest.mark.parametrize("check", ["bound", "partition", "sort", "subs", "inverse"])
def test_layout_holds_for_every_size_and_level(layout_report, check):
    rc, report = layout_report
    assert report.get(check) == check + " ok", report.get(check)


def test_layout_program_exit_status(layout_report):
    rc, report = layout_report
    assert rc == 0, report


def test_every_size_was_checked(layout_report):
    _, report = layout_report
    n = int(report["checked"].split()[1])
    # 1 .. 300,000 and five sizes around each 2^k * 4096 above that (k = 7 .. 10)
    assert n == 300_000 + 5 * 4, report["checked"]


def test_k_tree_local_takes_its_path_from_the_helper():
    """The kernel's path choice is the helper the program checks, not an expression of its
    own: the size estimate is gone from k_tree.hip and the guard on the sub-node count is there."""
    src = open(os.path.join(CSRC, "k_tree.hip")).read()
    assert re.search(r"sort_per\s*=\s*tree_local_sort_per\(n, l\)", src)
    assert re.search(r"nsub > kLocalPartSubs\)+\s*sort_per = kWaveSortPer", src)
    assert "max_sub" not in src
    hdr = open(os.path.join(CSRC, "tree.hpp")).read()
    assert "static_assert(kLocalMax / (2 * kLocalPartSubs) <= 64 * kWaveSortPer" in hdr
