#!/bin/bash
# The measurements of record for a tree, on one box (run on the GPU box from the repo root): tools/measure.sh TAG [suite]
# Results in $RESULTS_DIR (default: results/):
#   1. with "suite": the whole GPU test suite                                   -> gputest_TAG.txt
#   2. the bench line (bench.py --full)                                         -> bench_TAG.json
#   3. the same command under rocprofv3 --kernel-trace --stats                  -> kernel_stats_TAG.csv, bench_TAG_under_rocprof.json
#   4. the two PMC passes (FETCH_SIZE, WRITE_SIZE) of the bench's timed region  -> TAG_pmc_bench16g.txt
# Copy what is to be judged into profiles/ and add the traffic entry with tools/pmc_to_traffic.py (profiles/README.md).
tag=${1:-x}; root=$(pwd); export TMPDIR=/tmp; export RESULTS_DIR=${RESULTS_DIR:-$root/results}; res=$RESULTS_DIR; mkdir -p $res
if [ "$2" = suite ]; then
  ( timeout 2400 python3 -m pytest tests -q -m gpu -p no:cacheprovider < /dev/null 2>&1 | tail -8 ) > $res/gputest_$tag.txt; cat $res/gputest_$tag.txt
fi
bash tools/bench_profile.sh $tag
bash tools/pmc_bench.sh ${tag}_pmc_bench16g.txt
