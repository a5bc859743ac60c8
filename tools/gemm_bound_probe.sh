#!/bin/bash
# usage (GPU box): bash tools/gemm_bound_probe.sh [out-file]  -> the probe at the default clock (default file: measure_out/gemm_bound_probe.txt)
out=${1:-measure_out/gemm_bound_probe.txt}
mkdir -p "$(dirname "$out")"
echo "== default clocks" > $out
python tools/gemm_bound_probe.py >> $out 2>&1
cat $out
