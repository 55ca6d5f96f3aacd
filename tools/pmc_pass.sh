#!/bin/bash
# usage: tools/pmc_pass.sh NAME "COUNTER1 COUNTER2 ..." [GiB]   (run on the GPU box, from the repo root; one --pmc pass, nothing else traced)
# the counter CSVs and the log go to $RESULTS_DIR/NAME (default: results/), like pmc_bench.sh's
name=$1; ctrs=$2; gib=${3:-1}
root=$(pwd); export TMPDIR=/tmp; res=${RESULTS_DIR:-$root/results}; mkdir -p $res; cd /tmp
timeout 150 rocprofv3 --pmc $ctrs --output-format csv -d $res/$name -o p -- python3 $root/tools/bringup/gpu_compress_once.py $gib > $res/$name.log 2>&1 < /dev/null
cd $root; python3 tools/pmc_summarize.py $res/$name
