#!/bin/bash
# GPU box: full bench + rocprofv3 kernel-trace summary of the plain bench command.
#   bash tools/prof_bench.sh <tag>   -> $out/<tag>_bench.log, $out/<tag>_kernel_stats.txt
#   (out = $CTCLIP_OUT, default bench_out)
set -e
tag=${1:-run}
out=${CTCLIP_OUT:-bench_out}
mkdir -p $out
export TMPDIR=/tmp
timeout -k 10 300 python -u bench.py --full > $out/${tag}_bench.log 2>&1
rm -rf $out/prof_${tag}
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $out/prof_${tag} -o run --output-format rocpd -- \
  python3 -u bench.py --steps 5 --warmup 2 > $out/${tag}_prof_bench.log 2>&1
db=$(find $out/prof_${tag} -name '*.db' | head -1)
python tools/rocprof_summary.py "$db" 7 > $out/${tag}_kernel_stats.txt
python tools/rocprof_grid.py "$db" "" 7 > $out/${tag}_grid_stats.txt
python tools/rocprof_streams.py "$db" 200 > $out/${tag}_streams.txt || true
python tools/rocprof_timeline.py "$db" > $out/${tag}_timeline.txt || true
python tools/rocprof_seq.py "$db" > $out/${tag}_seq.txt || true
python tools/rocprof_copies.py "$db" 7 > $out/${tag}_copies.txt || true
rm -rf $out/prof_${tag}
