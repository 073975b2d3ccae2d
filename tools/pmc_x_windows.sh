#!/bin/bash
# Counters of the 128^3 fine-level SpMV on variant 17, direct gathers against the x-window launch mode (GPU box, repo root):
#   bash tools/pmc_x_windows.sh <rows per workgroup: 0 direct, 256, 512, 1024> <out.txt>
# One rocprofv3 --pmc pass per counter group over `python bench.py --gpus 1 --steps 20 --warmup 5` with the kernel pinned
# (SAENA_BENCH_VARIANT=17; SAENA_X_WINDOWS pins the mode), counters only -- no tracing in the same run.  Prints the mean per launch
# over the launches of the most-launched k_vidx / k_vidxw / k_vidxw_fast kernel: texture-addresser busy cycles, L1 accesses and pending-stall
# cycles (summed over the CUs), FETCH_SIZE (KiB as reported: x 2 on gfx950 for wide coalesced streams, tools/pmc_summarise.py),
# the waves' instruction counts, and -- of the cycles a wave spends issuing or waiting per instruction class -- whatever the box's
# counter list offers (asked of rocprofv3 first: a counter it does not name is left out, not tried).  VALU per wave and the share of
# the kernel's clocks the vector unit is busy are printed where their counters came back.
# A pass that fails ends the script: the passes after it would measure a box that has just shown it cannot be measured.
set -e
ROWS=${1:-0}; OUT=${2:-pmc_x_windows.txt}
D=$(mktemp -d)
export SAENA_PLAN_CACHE=off SAENA_BENCH_VARIANT=17
if [ "$ROWS" != "0" ]; then export SAENA_X_WINDOWS=$ROWS; fi
GROUPS_=("TA_TA_BUSY_sum TCP_TOTAL_CACHE_ACCESSES_sum GRBM_GUI_ACTIVE" "TCP_PENDING_STALL_CYCLES_sum FETCH_SIZE"
         "SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU")
# issue / wait cycles per class: only what the box lists, at most eight to a pass
WANT="SQ_ACTIVE_INST_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_SALU SQ_INST_CYCLES_VMEM SQ_WAIT_ANY SQ_WAIT_INST_LDS SQ_BUSY_CU_CYCLES SQ_CYCLES SQ_THREAD_CYCLES_VALU SQ_INSTS_VALU_MFMA_F64 SQ_INSTS_FLAT SQ_INSTS_SMEM SQ_LDS_BANK_CONFLICT"
if timeout -k 10 120 rocprofv3 --list-avail > $D/avail.txt 2>&1; then
    G=""; n=0
    for c in $WANT; do
        if grep -qw "$c" $D/avail.txt; then
            G="$G $c"; n=$((n+1))
            if [ $n -eq 8 ]; then GROUPS_+=("$G"); G=""; n=0; fi
        fi
    done
    if [ -n "$G" ]; then GROUPS_+=("$G"); fi
else
    echo "rocprofv3 --list-avail failed: only the fixed counter groups are collected" >&2
fi
i=0
for C in "${GROUPS_[@]}"; do
    i=$((i+1))
    if ! timeout -k 10 300 rocprofv3 --pmc $C --output-format csv -d $D/pass$i -- python3 bench.py --gpus 1 --steps 20 --warmup 5 > $D/pass$i.log 2>&1; then
        echo "pass $i ($C) failed; stopping.  The end of its log:" >&2
        tail -n 20 $D/pass$i.log >&2
        exit 1
    fi
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
        mean = {c: sum(v) / len(v) for c, v in vals.items()}
        if "SQ_WAVES" in mean and mean["SQ_WAVES"] > 0:
            for c in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_INSTS_VMEM_RD"):
                if c in mean: f.write(f"  {c + ' / SQ_WAVES':36s} {mean[c] / mean['SQ_WAVES']:.2f}\n")
        # GRBM_GUI_ACTIVE: the kernel's clocks, one count per launch.  SQ_ACTIVE_INST_VALU and SQ_BUSY_CYCLES come back summed over the
        # units that count them, so their quotient is a share of the time those units were busy, not of the kernel: both are printed.
        if "SQ_ACTIVE_INST_VALU" in mean and mean.get("SQ_BUSY_CYCLES", 0) > 0:
            f.write(f"  {'SQ_ACTIVE_INST_VALU / SQ_BUSY_CYCLES':36s} {mean['SQ_ACTIVE_INST_VALU'] / mean['SQ_BUSY_CYCLES']:.3f}\n")
        if "GRBM_GUI_ACTIVE" in mean:
            f.write(f"  {'kernel clocks (GRBM_GUI_ACTIVE)':36s} {mean['GRBM_GUI_ACTIVE']:.6g}\n")
    else:
        f.write("no k_vidx launches found\n")
print(open(out).read())
PY
