#!/usr/bin/env python
"""Two-sided summaries of an A/B of a context switch under rocprofv3 (round 8: option "stream_hints" through POI_TE_STREAM=1 / 0):
  <tag>_pmc_traffic.json    FETCH_SIZE / WRITE_SIZE per launch of every timed region of the training step, one block per side
                            (`rocprofv3 --pmc <counter>` alone - no tracing combined - one pass per counter and side)
  <tag>_kernel_stats.md     per-kernel time of `rocprofv3 --kernel-trace --stats`, both sides next to each other
usage: python tools/pmc_ab.py <dir with fetch_on fetch_off write_on write_off stats_on stats_off> <tag>
The counters' units and the gfx950 correction (FETCH_SIZE doubled) are those of tools/make_profiles.py."""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict

src, tag = sys.argv[1], sys.argv[2]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")
CMD = "python bench.py --gpus 1 --steps 20 --warmup 2 --no-cpu-baseline --no-quality --no-secondary --no-exact --no-x1 --no-bpr --no-projection --no-eval"
# timed regions of the training step -> kernels (name prefixes, as tools/make_profiles.py)
REGION = {"te_gemm_ax": ["te_xpack_kernel", "te_xwpackd_kernel", "te_xztab_kernel", "te_gemmx_kernel", "te_xcount_kernel", "te_xassign_kernel"],
          "te_rec_fwd": ["te_rec_fwdx_kernel", "te_rec_fwdxi_kernel", "te_rec_fwd1x_kernel", "te_rec_fwd1xi_kernel"],
          "te_head": ["te_head3_kernel"], "te_rec_bwd": ["te_rec_bwd16t_kernel", "te_rec_bwd1_kernel"],
          "te_psum": ["te_pcount_kernel", "te_passign_kernel", "te_psum_kernel", "te_pfin_kernel"], "te_wgrad": ["te_wgrad_kernel"],
          "te_gemm_dx": ["te_gemm_ntk_kernel<false, false"], "te_dsum": ["te_dprep_kernel", "te_dsum_kernel"],
          "te_scatter": ["te_reduce_kernel", "te_hot_reduce_kernel", "te_hot_apply_kernel"]}


def short(name):
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*", "", name).replace("poi::", "")


def find(sub, pat):
    g = glob.glob(os.path.join(src, sub, "**", pat), recursive=True)
    assert g, (sub, pat)
    return g[0]


def counters(sub, counter):
    acc, calls = defaultdict(float), defaultdict(set)
    for r in csv.DictReader(open(find(sub, "*counter_collection.csv"))):
        if r["Counter_Name"] == counter:
            k = short(r["Kernel_Name"])
            acc[k] += float(r["Counter_Value"]); calls[k].add(r["Dispatch_Id"])
    return acc, {k: len(v) for k, v in calls.items()}


def side(s):
    fa, fc = counters("fetch_" + s, "FETCH_SIZE")
    wa, wc = counters("write_" + s, "WRITE_SIZE")
    out = {}
    for reg, pats in REGION.items():
        fk = [k for k in fa if any(k.startswith(p) for p in pats)]
        wk = [k for k in wa if any(k.startswith(p) for p in pats)]
        if not fk:
            continue
        nf, nw = max(fc[k] for k in fk), max([wc[k] for k in wk], default=1)
        fetch, write = sum(fa[k] for k in fk) / nf, sum(wa[k] for k in wk) / nw
        out[reg] = {"kernels": sorted(fk), "launches": nf, "launches_write_pass": nw, "fetch_kb_raw": fetch, "write_kb": write,
                    "hbm_bytes_per_launch": (2.0 * fetch + write) * 1024.0}
    return out


doc = {"config": CMD + "  (gowalla shape, 12500 users per launch)",
       "note": "rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE, each in a pass of its own with no tracing combined; hints_on: POI_TE_STREAM=1 (option "
               "\"stream_hints\" 1, the default), hints_off: POI_TE_STREAM=0; counter unit KB (x 1024); FETCH_SIZE is doubled in hbm_bytes_per_launch "
               "(gfx950 reports half of wide coalesced reads); per launch of the TIMED REGION (sum over its kernels), each pass normalised by its own launch count",
       "hints_on": side("on"), "hints_off": side("off")}
json.dump(doc, open(os.path.join(P, tag + "_pmc_traffic.json"), "w"), indent=1)

st = {}
for s in ("on", "off"):
    st[s] = {short(r["Name"]): r for r in csv.DictReader(open(find("stats_" + s, "*kernel_stats.csv")))}
with open(os.path.join(P, tag + "_kernel_stats.md"), "w") as f:
    f.write("# %s - rocprofv3 --kernel-trace --stats of `%s`\n\n" % (tag, CMD))
    f.write("Gowalla-shape synthetic (100 k POIs, 50 k users, L <= 50, D = 128, 200 bins), one MI355X, 22 training epochs of 4 launches (12500 users each).\n"
            "Left: the build as committed (option \"stream_hints\" 1: the tile kernels of the forward recurrence are the `_nt` instances); right: the same build\n"
            "with POI_TE_STREAM=0 (plain stores).  One pass each; the trace serialises the two streams' kernels (docs/NOTEBOOK.md, round 7).\n\n")
    f.write("| kernel (hints on) | calls | avg us | % | avg us, hints off |\n|---|---|---|---|---|\n")
    for k, r in sorted(st["on"].items(), key=lambda kv: -float(kv[1]["TotalDurationNs"])):
        if float(r["Percentage"]) < 0.5:
            continue
        o = st["off"].get(k) or st["off"].get(k.replace("_kernel_nt<128, true>", "_kernel<128, true, false>").replace("_kernel_nt<128>", "_kernel<128, false>"))
        f.write("| `%s` | %s | %.1f | %.2f | %s |\n" % (k, r["Calls"], float(r["AverageNs"]) / 1e3, float(r["Percentage"]), ("%.1f" % (float(o["AverageNs"]) / 1e3)) if o else "-"))
print("wrote", [x for x in os.listdir(P) if x.startswith(tag)])
