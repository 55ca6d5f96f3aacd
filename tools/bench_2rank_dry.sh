#!/bin/bash
# run on the GPU box from the repo root: control-flow dry run of bench.py --gpus 2 with both ranks on the one GPU (gloo + host transport);
# --full: the routed answers of the last step are spot-checked against every owner's corpus. Results in $RESULTS_DIR (default: results/)
root=$(pwd); res=${RESULTS_DIR:-$root/results}; mkdir -p $res
ZRA_BENCH_ONE_GPU=1 timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29531 \
  bench.py --gpus 2 --steps 2 --warmup 1 --size-gib 2 --queries 200000 --full > $res/bench_2rank_dry.json 2> $res/bench_2rank_dry.err < /dev/null
echo rc=$?
tail -c 900 $res/bench_2rank_dry.json
tail -3 $res/bench_2rank_dry.err
