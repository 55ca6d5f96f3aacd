#!/bin/bash
# run on the GPU box from the repo root: the decode pass of the flagship step, another build of the library against the in-tree one,
# alternating processes on one box (the pattern of tools/ab.sh and tools/dec_ab.sh):
#   tools/dec_front_ab.sh OTHER_LIB [REPS] [trace]
#     OTHER_LIB   a libzra_amd.so built from the commit to compare with (loaded through ZRA_AMD_LIB, zra_amd/__init__.py)
#     REPS        processes per build (default 4): bench.py --gpus 1 --steps 10 --warmup 3; the first pair also writes --dump-outputs
#                 and every array of the two dumps is compared
#     trace       afterwards one process per build under rocprofv3 --kernel-trace --stats (bench.py --steps 3 --warmup 1 --timed-only;
#                 no counters in these runs): the zra_dec_* rows and the whole table as OUT/dec_front_kernel_stats_{other,tree}.csv
# Output: OUT/dec_front_ab.txt (OUT = $ZRA_AB_OUT, default results/ under the repo root) — per process the headline, whole_pass_ms,
# the stage times and parse + huf; then per build the mean and the spread (max - min) of whole_pass_ms and of parse + huf, and the
# verdict "difference > 2 x the other build's spread".
root=$(pwd); out=${ZRA_AB_OUT:-$root/results}; mkdir -p $out; export TMPDIR=/tmp
other=$1; reps=${2:-4}; trace=$3
[ -f "$other" ] || { echo "usage: tools/dec_front_ab.sh OTHER_LIB [REPS] [trace]"; exit 2; }
txt=$out/dec_front_ab.txt; : > $txt
pick='
import json, sys
j = json.loads(open(sys.argv[1]).read().strip().split("\n")[-1])
r = j["roofline_ra"]; s = r["stage_ms_per_pass"]
print("value %.3f ms_per_step %.2f ra_us_per_query %.3f whole_pass_ms %.3f parse %.3f huf %.3f chain %.3f exec %.3f parse+huf %.3f" % (
    j["value"], j["ms_per_step"], j["ra_us_per_query"], r["whole_pass_ms"], s["parse_ms"], s["huf_ms"], s["chain_ms"], s["exec_ms"], s["parse_ms"] + s["huf_ms"]))
'
use() { if [ $1 = other ]; then export ZRA_AMD_BRINGUP=1 ZRA_AMD_LIB=$other; else unset ZRA_AMD_BRINGUP ZRA_AMD_LIB; fi; }
for r in $(seq 1 $reps); do
  for v in other tree; do
    use $v
    extra=""; [ $r = 1 ] && extra="--dump-outputs /tmp/dec_front_dump_$v"
    timeout -k 10 300 python3 bench.py --gpus 1 --steps 10 --warmup 3 $extra > $out/dec_front_${v}_$r.json 2> $out/dec_front_${v}_$r.err < /dev/null
    rc=$?
    [ $rc -ne 0 ] && { echo "$v $r: exit status $rc" | tee -a $txt; tail -20 $out/dec_front_${v}_$r.err; exit $rc; }
    echo "$v $r: $(python3 -c "$pick" $out/dec_front_${v}_$r.json)" | tee -a $txt
  done
done
unset ZRA_AMD_BRINGUP ZRA_AMD_LIB
python3 - $txt /tmp/dec_front_dump_other /tmp/dec_front_dump_tree <<'EOF' | tee -a $txt
import os, re, sys
import numpy as np
rows = {"other": [], "tree": []}
for line in open(sys.argv[1]):
    m = re.match(r"(other|tree) \d+: .*whole_pass_ms ([\d.]+) .*parse\+huf ([\d.]+)", line)
    if m:
        rows[m.group(1)].append((float(m.group(2)), float(m.group(3))))
for k, name in ((0, "whole_pass_ms"), (1, "parse+huf ms")):
    o = [r[k] for r in rows["other"]]; t = [r[k] for r in rows["tree"]]
    spread = max(o) - min(o)
    print("%-14s other mean %.3f spread %.3f | tree mean %.3f spread %.3f | difference %.3f %s 2 x the other build's spread (%.3f)" % (
        name, np.mean(o), spread, np.mean(t), max(t) - min(t), np.mean(o) - np.mean(t), ">" if np.mean(o) - np.mean(t) > 2 * spread else "NOT >", 2 * spread))
a, b = sys.argv[2], sys.argv[3]
na, nb = sorted(os.listdir(a)), sorted(os.listdir(b))
bad = na != nb
for n in na:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    eq = x.shape == y.shape and bool(np.array_equal(x, y))
    bad |= not eq
    print("  --dump-outputs %-24s %-12s %s" % (n, x.shape, "equal" if eq else "DIFFERENT"))
print("outputs of the two builds: " + ("DIFFERENT" if bad else "every array equal"))
EOF
[ "$trace" = trace ] || exit 0
for v in other tree; do
  use $v
  rm -rf /tmp/dec_front_prof_$v
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/dec_front_prof_$v -o k -- python3 bench.py --gpus 1 --steps 3 --warmup 1 --timed-only > $out/dec_front_trace_$v.json 2> $out/dec_front_trace_$v.err < /dev/null
  rc=$?
  [ $rc -ne 0 ] && { echo "$v under rocprofv3: exit status $rc" | tee -a $txt; exit $rc; }
  k=$(find /tmp/dec_front_prof_$v -name '*kernel_stats.csv' | head -1)
  [ -n "$k" ] || continue
  cp "$k" $out/dec_front_kernel_stats_$v.csv
  echo "== $v under rocprofv3 --kernel-trace --stats: kernel, calls, total ns, average ns" | tee -a $txt
  grep "zra_dec_" "$k" | cut -d, -f1-4 | tee -a $txt
done
unset ZRA_AMD_BRINGUP ZRA_AMD_LIB
