#!/bin/bash
# run on the GPU box from the repo root: the headline bench line (--full), then the same command under rocprofv3 --kernel-trace --stats;
# results in $RESULTS_DIR (default: results/) as bench_$1.json, bench_$1_under_rocprof.json, kernel_stats_$1.csv
tag=${1:-x}
root=$(pwd); export TMPDIR=/tmp
res=${RESULTS_DIR:-$root/results}; mkdir -p $res
timeout 900 python3 $root/bench.py --full > $res/bench_$tag.json 2> $res/bench_$tag.err < /dev/null
tail -c 600 $res/bench_$tag.json
cd /tmp; rm -rf /tmp/kst_$tag
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/kst_$tag -o k -- python3 $root/bench.py --full --no-cpu-baseline > $res/bench_${tag}_under_rocprof.json 2>/dev/null < /dev/null
f=$(find /tmp/kst_$tag -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" $res/kernel_stats_$tag.csv && head -8 $res/kernel_stats_$tag.csv | cut -c1-150
