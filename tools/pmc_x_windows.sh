#!/bin/bash
# Counters of the 128^3 fine-level SpMV on variant 17, direct gathers against the x-window launch mode (GPU box, repo root):
#   bash tools/pmc_x_windows.sh <rows per workgroup: 0 direct, 256, 512, 1024> <out.txt>
# One rocprofv3 --pmc pass per counter group over `python bench.py --gpus 1 --steps 20 --warmup 5` with the kernel pinned
# (SAENA_BENCH_VARIANT=17; SAENA_X_WINDOWS pins the mode), counters only -- no tracing in the same run.  Prints the mean per launch
# over the launches of the most-launched k_vidx / k_vidxw kernel: texture-addresser busy cycles, L1 accesses and pending-stall
# cycles (summed over the CUs), FETCH_SIZE (KiB as reported: x 2 on gfx950 for wide coalesced streams, tools/pmc_summarise.py),
# and the waves' instruction counts.
set -e
ROWS=${1:-0}; OUT=${2:-pmc_x_windows.txt}
D=$(mktemp -d)
export SAENA_PLAN_CACHE=off SAENA_BENCH_VARIANT=17
if [ "$ROWS" != "0" ]; then export SAENA_X_WINDOWS=$ROWS; fi
GROUPS_=("TA_TA_BUSY_sum TCP_TOTAL_CACHE_ACCESSES_sum GRBM_GUI_ACTIVE" "TCP_PENDING_STALL_CYCLES_sum FETCH_SIZE"
         "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU")
i=0
for C in "${GROUPS_[@]}"; do
    i=$((i+1))
    timeout -k 10 300 rocprofv3 --pmc $C --output-format csv -d $D/pass$i -- python3 bench.py --gpus 1 --steps 20 --warmup 5 > $D/pass$i.log 2>&1 || echo "pass $i ($C) failed" >> $D/failed.txt
done
python3 - "$D" "$OUT" "$ROWS" <<'PY'
import csv, glob, sys
from collections import defaultdict
d, out, rows_per_wg = sys.argv[1], sys.argv[2], sys.argv[3]
rows = []
for f in sorted(glob.glob(d + "/pass*/**/*counter_collection.csv", recursive=True)):
    rows += list(csv.DictReader(open(f)))
names = defaultdict(int)
for r in rows:
    if "sk::k_vidx" in r["Kernel_Name"]: names[(r["Kernel_Name"], r["Grid_Size"], r.get("Workgroup_Size", ""))] += 1
with open(out, "w") as f:
    f.write(f"SAENA_BENCH_VARIANT=17, x windows {rows_per_wg}: rocprofv3 --pmc passes of python bench.py --gpus 1 --steps 20 --warmup 5; mean per launch\n")
    if names:
        k = max(names, key=names.get)
        vals = defaultdict(list)
        for r in rows:
            if (r["Kernel_Name"], r["Grid_Size"], r.get("Workgroup_Size", "")) == k: vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
        f.write(f"{k[0]} grid {k[1]} workgroup {k[2]}\n")
        for c, v in sorted(vals.items()):
            f.write(f"  {c:36s} n={len(v):5d} mean={sum(v) / len(v):.6g} min={min(v):.6g} max={max(v):.6g}\n")
    else:
        f.write("no k_vidx launches found\n")
print(open(out).read())
PY
