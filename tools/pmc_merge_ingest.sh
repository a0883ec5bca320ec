#!/bin/bash
# SQ counters of ct::merge_ingest_kernel (planar and interleaved, C2 shape) next to the two launches it replaces and the
# code-route merge: two rocprofv3 --pmc passes of their own (no trace domains mixed in) over
# `tools/merge_ingest_bench.py --profile 6`, then per-dispatch averages per kernel.
#   tools/pmc_merge_ingest.sh OUTPUT_DIR        (run from the repository root)
set -e
O=${1:?output directory}
mkdir -p "$O"
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE \
  -d "$O/p1" --output-format csv -- python tools/merge_ingest_bench.py --profile 6 > "$O/p1.log" 2>&1
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM \
  -d "$O/p2" --output-format csv -- python tools/merge_ingest_bench.py --profile 6 > "$O/p2.log" 2>&1
python3 - "$O" <<'PY'
import collections, csv, glob, sys
for p in ("p1", "p2"):
    for f in glob.glob(f"{sys.argv[1]}/{p}/**/*counter_collection.csv", recursive=True):
        agg, cnt, seen = collections.defaultdict(lambda: collections.defaultdict(float)), collections.Counter(), set()
        for r in csv.DictReader(open(f)):
            k = r["Kernel_Name"]
            if not any(w in k for w in ("merge_ingest_kernel", "merge_kernel", "merge_pivot_kernel", "ingest_planar_kernel", "ingest_packed3_kernel")):
                continue
            k = k.split("(")[0][-70:]
            agg[k][r["Counter_Name"]] += float(r["Counter_Value"])
            if (r["Dispatch_Id"], k) not in seen:
                seen.add((r["Dispatch_Id"], k))
                cnt[k] += 1
        for k in sorted(agg):
            print(p, k, "dispatches", cnt[k], {c: "%.4g" % (v / cnt[k]) for c, v in sorted(agg[k].items())})
PY
