#!/bin/bash
# usage: tools/trace_pass.sh <tag> <bench args...>  -- rocprofv3 --kernel-trace --stats, keeps only the per-kernel stats CSV + bench line
export TMPDIR=/tmp; cd "$(dirname "$0")/.."
OUT=${OUT:?set OUT to the directory for the results}; mkdir -p "$OUT"
tag=$1; shift
mkdir -p /tmp/trace
timeout 200 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/trace/$tag -o t -- python bench.py "$@" > /tmp/trace/$tag.log 2>&1 || echo "trace failed"
f=$(ls /tmp/trace/$tag/*kernel_stats.csv 2>/dev/null | head -1)
[ -n "$f" ] && cp "$f" $OUT/${tag}_kernel_stats.csv
grep '^{' /tmp/trace/$tag.log | tail -1 > $OUT/${tag}_bench.json
ls /tmp/trace/$tag | head
