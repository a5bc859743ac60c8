#!/bin/bash
# usage (GPU box): tools/refresh_measure.sh <round-tag> [out-dir]   -> <out-dir>/<tag>_bench_line_*.json (default out-dir: measure_out/);
# the profiles, counters and timings go to the output folder of tools/prof.sh
# The part of tools/final_measure.sh that a change to the step's non-GEMM kernels touches: every bench line, the reproducibility check,
# the two kernel profiles, the launch count, the memory-traffic counters, the attention timings.  (The GEMM probes are unaffected.)
tag=${1:-r04}
# the bench lines (every block of the line: --full) go to the directory named by the second argument
out=${2:-measure_out}
mkdir -p "$out"
mkdir -p gpurun_out
python bench.py --full 2>/dev/null | tail -1 > "$out"/${tag}_bench_line_default.json
for dt in f16x2 f16 f16x2s; do
  python bench.py --full --dtype $dt --no-cpu-baseline --no-modes 2>/dev/null | tail -1 > "$out"/${tag}_bench_line_$dt.json
done
for b in 16 32 64; do
  python bench.py --full --batch $b --no-cpu-baseline --no-modes --steps 12 --warmup 3 2>/dev/null | tail -1 > "$out"/${tag}_bench_line_b$b.json
done
python bench.py --full --gpus 1 --spawn 2>/dev/null | tail -1 > "$out"/${tag}_bench_line_spawn1.json
for ps in RGBNT100 MSVR310 SYNTH4L; do
  python bench.py --full --preset $ps --no-cpu-baseline --no-modes 2>/dev/null | tail -1 > "$out"/${tag}_bench_line_$(echo $ps | tr A-Z a-z).json
done
DBG_B=128 python tools/repro_check.py > gpurun_out/${tag}_repro_check.txt 2>&1
bash tools/prof.sh ${tag} --no-replay --no-h2d --no-modes --no-eval > gpurun_out/${tag}_prof.txt 2>&1
cp gpurun_out/prof_${tag}/kernel_stats.csv gpurun_out/${tag}_bench_kernel_stats.csv
EDITOR_WGRAD_STREAM=0 bash tools/prof.sh ${tag}s --no-replay --no-h2d --no-modes --no-eval > gpurun_out/${tag}_prof_serial.txt 2>&1
cp gpurun_out/prof_${tag}s/kernel_stats.csv gpurun_out/${tag}_bench_kernel_stats_serial.csv
bash tools/launch_count.sh ${tag} > /dev/null 2>&1
TAG=${tag} bash tools/pmc_traffic.sh > gpurun_out/${tag}_pmc_traffic.log 2>&1
python tools/attn_bench.py > gpurun_out/${tag}_attn_bench.txt 2>&1
head -c 700 "$out"/${tag}_bench_line_default.json; echo
for f in f16x2 f16x2s f16 rgbnt100 msvr310 synth4l b16 b32 b64 spawn1; do head -c 330 "$out"/${tag}_bench_line_$f.json; echo; done
tail -4 gpurun_out/${tag}_repro_check.txt
tail -3 gpurun_out/${tag}_pmc_traffic.log
