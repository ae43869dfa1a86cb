"""Static guard on the capped top-K kernels (csrc/capped.hip): the walk keeps the rows' and the item tile's fragments in registers
beside the 32 x 32 accumulator and, in the rare part, a list entry with its label per lane; the merges hold two lists over the lanes -
all of it is only worth having while none of it lives in scratch memory.  Reads the register / scratch / LDS table of
tools/kernel_resources.py (the compiler's own resource remarks): sizes only, no instruction is searched for.  Skipped when hipcc is not
installed."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "point-of-interest-recommendation_amd", "csrc", "capped.hip")

WALK = ["capped_walk_kernel<%s, %s>" % (d8, geo) for d8 in ("4, true", "8, true", "16, false", "32, false") for geo in ("true", "false")]
SMALL = ["labels_hist_kernel", "labels_fill_kernel"]
LISTS = ["capped_scores_kernel", "capped_slices_merge_kernel"]


@pytest.fixture(scope="module")
def table():
    if not (os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc")):
        pytest.skip("hipcc not installed")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), SRC], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = {}
    for line in out.stdout.splitlines()[1:]:
        m = re.match(r"(.*?)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1).strip()] = dict(zip(("vgpr", "agpr", "scratch", "occ", "lds"), map(int, m.groups()[1:])))
    return rows


def test_the_capped_kernels_compile_without_scratch(table):
    for k in WALK + SMALL + LISTS:
        assert k in table, "kernel %s not found in %s (have %s)" % (k, SRC, sorted(table))
        print(k, table[k])
        assert table[k]["scratch"] == 0, (k, table[k])


def test_the_walk_leaves_room_for_its_lists(table):
    """Static LDS of the walk beside its 48 KiB of dynamic lists (and 32 KiB of thresholds with the distance term): a few KiB."""
    for k in WALK:
        assert table[k]["lds"] <= 4096, (k, table[k])


def test_the_small_kernels_leave_the_cu_to_many_workgroups(table):
    for k in SMALL:
        assert table[k]["occ"] >= 8 and table[k]["lds"] <= 2048, (k, table[k])
    for k in LISTS:
        assert table[k]["occ"] >= 4 and table[k]["lds"] <= 2048, (k, table[k])
