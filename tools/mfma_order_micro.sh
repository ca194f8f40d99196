#!/bin/bash
# The matrix cores' ceiling per MFMA issue order (tools/micro/mfma_order.hip): wall-clock rate, then the in-load clock from
# a counter pass of its own (the `clk` set of tools/pmc_workload.sh; counters are never combined with tracing other than
# the kernel trace that names the launches).  Results: $OUT/micro.txt (OUT defaults to tools/micro/out)
#   [OUT=dir] tools/mfma_order_micro.sh [rounds]
# A step that fails or runs past its time limit ends the script: nothing more is started on the GPU.
set -o pipefail
export TMPDIR=/tmp
cd "$(dirname "$0")/.."
ROUNDS=${1:-3}
out=${OUT:-$PWD/tools/micro/out}
mkdir -p $out
[ -x tools/micro/mfma_order ] || /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -o tools/micro/mfma_order tools/micro/mfma_order.hip || exit 1
{
  echo "== wall-clock rate, $ROUNDS interleaved rounds (TFLOP/s per launch)"
  timeout -k 10 240 ./tools/micro/mfma_order --rounds $ROUNDS || { echo "the rate run failed (rc $?)"; exit 1; }
} 2>&1 | tee $out/micro.txt
[ ${PIPESTATUS[0]} = 0 ] || exit 1
rm -rf $out/pmc
timeout -k 10 240 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES --kernel-trace --output-format csv -d $out/pmc -o run -- ./tools/micro/mfma_order --quick > $out/pmc.log 2>&1 || { echo "the counter pass failed (rc $?), see $out/pmc.log" | tee -a $out/micro.txt; exit 1; }
python3 - $out/pmc <<'PY' | tee -a $out/micro.txt
import csv, glob, re, sys, collections
files = glob.glob(sys.argv[1] + '/**/run_counter_collection.csv', recursive=True)
agg = collections.defaultdict(lambda: collections.defaultdict(list))
for f in files:
    for r in csv.DictReader(open(f)):
        m = re.search(r'k_order<(\d), (\w+)>', r['Kernel_Name']) or re.search(r'k_orderILi(\d)ELb(\d)', r['Kernel_Name'])
        if m:
            key = ('abcd'[int(m.group(1))], 'dense' if m.group(2) in ('true', '1') else 'post-ReLU')
            agg[key][r['Counter_Name']].append((float(r['Counter_Value']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
print('== counter pass (launches serialised; the last launch of each order): in-load clock = GRBM_GUI_ACTIVE / 8 / duration')
for key in sorted(agg, key=lambda k: (k[1] != 'post-ReLU', k[0])):
    g, t = agg[key]['GRBM_GUI_ACTIVE'][-1]
    m, _ = agg[key]['SQ_VALU_MFMA_BUSY_CYCLES'][-1]
    cyc = g / 8
    print('%s %-9s launch_ms %.2f clock_GHz %.3f cycles %.0f mfma_busy %.3f' % (key[0], key[1], t / 1e6, cyc / t, cyc, m / (cyc * 1024)))
PY
