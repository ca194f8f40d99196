#!/bin/bash
# Round-6 evidence, run on the GPU box from the repo root.  Copies what is judged into profiles/r6/ (tracked):
#   bench.json / bench_full.json                 the default command's ONE line (<= 4 KB) and its full record
#   bench_driver_cmd.json / bench_full_driver_cmd.json   the driver's command (--gpus 1 --steps 20 --warmup 5)
#   kernel_stats_default_bench.csv               rocprofv3 --kernel-trace --stats of the default command (its average
#                                                duration of the dominant kernel must agree with roofline.avg_launch_ms)
#   kernel_stats_seam_default.csv                the same of the seam as hip.rs runs it by default: one kernel, no decode launch
#   mfma_busy.txt                                clock / MFMA-busy / SQ / LDS counter passes of the dominant kernels
#   FETCH_SIZE / WRITE_SIZE passes (-> profiles/hbm_traffic.json) of every dominant kernel whose source changed this round
#   (kz_board_conv.hip: the staging-store map; kz_conv_heads.hpp: the wave-count guard of the in-launch decode)
export TMPDIR=/tmp
O=gpurun_out/r6
mkdir -p $O profiles/r6
STEPS=4 WARMUP=1 bash tools/pmc_traffic.sh go19-40x256 f16
STEPS=3 WARMUP=1 bash tools/pmc_traffic.sh go19-40x256 f32split16
STEPS=30 WARMUP=5 bash tools/pmc_traffic.sh chess-20x256 f32split16
STEPS=60 WARMUP=10 bash tools/pmc_traffic.sh ataxx-8x128 f32
STEPS=60 WARMUP=10 bash tools/pmc_traffic.sh ataxx-8x128 f32split16
STEPS=30 WARMUP=5 bash tools/pmc_traffic.sh chess-20x256 f16
python3 bench.py --full > $O/bench.json 2> $O/bench.err; cp bench_full.json $O/bench_full.json
python3 bench.py --gpus 1 --steps 20 --warmup 5 > $O/bench_driver_cmd.json 2> $O/bench_driver_cmd.err; cp bench_full.json $O/bench_full_driver_cmd.json
wc -c $O/bench.json $O/bench_driver_cmd.json
rm -rf $O/stats
KZ_BENCH_FULL_RECORD=$PWD/$O/stats_bench_full.json rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o run -- python3 bench.py --full --steps 2000 --repeats 3 --no-cpu-baseline --no-seam > $O/stats_bench.json 2> $O/stats.log
f=$(ls -S $(find $O/stats -name "*kernel_stats.csv") | head -1)
cp "$f" $O/kernel_stats_default_bench.csv
rm -rf $O/stats
bash tools/bench_executor_r5.sh 1 > /dev/null 2>&1   # (builds the executable and the model file)
rm -rf $O/stats_seam
# work=real, 1 executor thread, depth 3, device decode, 0 helpers: hip.rs's default since round 6
KZ_BENCH_CLEAN_EXIT=1 timeout 120 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_seam -o run -- tests/cpp/build/bench_executor /tmp/chess20x256.kzm 3 1 6 256 8 f16 3 1 0 real 0 > $O/stats_seam.json 2> $O/stats_seam.log
f=$(find $O/stats_seam -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $O/kernel_stats_seam_default.csv || echo "no kernel stats of the seam run" > $O/kernel_stats_seam_default.csv
rm -rf $O/stats_seam
python3 tools/show_bench.py $O/bench_full.json | cut -c1-260
head -12 $O/kernel_stats_default_bench.csv | cut -c1-170
cat $O/kernel_stats_seam_default.csv | cut -c1-170
: > $O/mfma_busy.txt
for w in "chess-20x256 f16 30" "chess-20x256 f32split16 20" "ataxx-8x128 f32 60" "go19-40x256 f16 3" "go19-40x256 f32split16 2"; do
  set -- $w
  bash tools/pmc_workload.sh $1 $2 $3 2>&1 | grep -v "^$" >> $O/mfma_busy.txt
done
cat $O/mfma_busy.txt
cp $O/bench.json $O/bench_full.json $O/bench_driver_cmd.json $O/bench_full_driver_cmd.json $O/kernel_stats_default_bench.csv $O/kernel_stats_seam_default.csv $O/mfma_busy.txt profiles/r6/
mkdir -p $O/pmc
for d in gpurun_out/pmc_traffic_*_FETCH_SIZE gpurun_out/pmc_traffic_*_WRITE_SIZE; do
  f=$(find $d -name "*counter_collection.csv" 2>/dev/null | head -1); [ -n "$f" ] && cp "$f" $O/pmc/$(basename $d).csv
done
cp profiles/hbm_traffic.json $O/hbm_traffic.json
