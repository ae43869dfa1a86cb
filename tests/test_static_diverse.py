"""Static guard on the diversified recommendation kernels (csrc/diverse.hip): the pool kernel keeps the rows' and the item tile's
fragments in registers beside the 32 x 32 accumulator, as group_kernel does, and is only worth having while none of that lives in scratch
memory; the split path's merge (csrc/topk_merge.hip) and the re-rank kernel are held to the same.  Reads every template instance's private segment size and spill count from
the library's gfx950 code objects (tools/scan_waits.py, as tests/test_static_group.py does): sizes only, no instruction is searched for.
Skipped when the ROCm binary tools are not installed."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("scan_waits", os.path.join(ROOT, "tools", "scan_waits.py"))
scan_waits = importlib.util.module_from_spec(spec)
spec.loader.exec_module(scan_waits)

KERNELS = (["diverse_pool_kernel<%s, %s>" % (d8, geo) for d8 in ("4, true", "8, true", "16, false", "32, false") for geo in ("true", "false")]
           + ["topk_slices_merge_kernel<64>"] + ["diverse_rerank_kernel<%s>" % ge for ge in ("true, true", "true, false", "false, true")])


@pytest.fixture(scope="module")
def found(tmp_path_factory):
    import poi_amd
    poi_amd.build.build_lib()                      # (no-op when the library is up to date)
    if not scan_waits.available():
        pytest.skip("llvm-objdump / clang-offload-bundler not installed")
    tmp = str(tmp_path_factory.mktemp("scan"))
    recs = {r["kernel"]: r for r in scan_waits.scan(["diverse_pool_kernel", "topk_slices_merge_kernel", "diverse_rerank_kernel"], tmp=tmp) if "loop" not in r}
    scratch = {}
    for co in scan_waits.code_objects(tmp):
        notes = subprocess.run([scan_waits.LLVM + "/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
        blocks = notes.split("  - .agpr_count:")[1:]
        names = scan_waits.demangle([re.search(r"\.name:\s+(\S+)", b).group(1) for b in blocks])
        for b in blocks:
            m = re.search(r"\.private_segment_fixed_size:\s+(\d+)", b)
            scratch[names[re.search(r"\.name:\s+(\S+)", b).group(1)]] = int(m.group(1)) if m else 0
    return recs, scratch


def test_the_diverse_kernels_compile_without_scratch(found):
    recs, scratch = found
    for k in KERNELS:
        assert k in recs and k in scratch, "kernel %s not found in the library" % k
        print(k, recs[k], "scratch", scratch[k])
        assert scratch[k] == 0 and recs[k]["spill"] == 0, (k, scratch[k], recs[k])
