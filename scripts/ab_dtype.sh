#!/bin/bash
# f64 against 'f32x' (scripts/ab_dtype.py) at the two shapes of profiles/r09_f32x.log, then a kernel trace of each dtype in a run of its own.
# Every GPU step runs under its own time limit and the script ends at the first one that fails.      bash scripts/ab_dtype.sh [out_dir]
cd "$(dirname "$0")/.." || exit 1
OUT=${1:-profile_out/ab_dtype}
mkdir -p "$OUT"
timeout -k 10 240 python3 scripts/ab_dtype.py --side 512 --points 500 --walkers 1024 > "$OUT/ab_512.log" 2>&1 || { tail -n 30 "$OUT/ab_512.log"; exit 1; }
cat "$OUT/ab_512.log"
timeout -k 10 840 python3 scripts/ab_dtype.py --side 1024 --points 1000 --walkers 8192 --steps 40 --regions 7 > "$OUT/ab_1024.log" 2>&1 || { tail -n 30 "$OUT/ab_1024.log"; exit 1; }
cat "$OUT/ab_1024.log"
for dt in f64 f32x; do
    rm -rf "$OUT/trace_$dt"
    timeout -k 10 200 rocprofv3 --kernel-trace --stats -d "$OUT/trace_$dt" -o t --output-format csv -- \
        python3 scripts/ab_dtype.py --side 512 --points 500 --walkers 1024 --dtypes $dt --regions 2 --steps 200 > "$OUT/trace_$dt.log" 2>&1 || { tail -n 30 "$OUT/trace_$dt.log"; exit 1; }
    f=$(find "$OUT/trace_$dt" -name '*kernel_stats.csv' | head -n 1)
    echo "== rocprofv3 kernel stats, $dt"
    head -n 5 "$f"
done
