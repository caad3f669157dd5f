#!/bin/bash
# builds tools/kw_bench (product objects), tools/kw_bench_trace (kernels_gemm_kw.hip with -DAPRIL_GEMM_TRACE: s_memtime stamps) and
# tools/kw_bench_ablate (the same with -DAPRIL_KW_ABLATE: the measurement-only forms APRIL_GEMM_DEBUG=3..11 of the compiler-scheduled
# K loop) from the repository root
set -e
cd "$(dirname "$0")/.."
C=april_asr_amd/csrc
make -C $C -j8 >/dev/null
HIPCC=/opt/rocm/bin/hipcc
T=$(mktemp -d)                       # (objects in a private directory: several users may build at once)
trap 'rm -rf "$T"' EXIT
$HIPCC --offload-arch=gfx950 -O2 -std=c++17 -I$C -c tools/kw_bench.hip -o $T/kw_bench.o
OBJS="$C/build/kernels_gemm.o $C/build/kernels_gemm_tile.o $C/build/kernels_gemm_pp.o $C/build/kernels_gemm_pw.o $C/build/kernels_recur.o $C/build/kernels_misc.o"
$HIPCC --offload-arch=gfx950 $T/kw_bench.o $OBJS $C/build/kernels_gemm_kw.o -o tools/kw_bench
$HIPCC -O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -DAPRIL_GEMM_TRACE -I$C -c $C/kernels_gemm_kw.hip -o $T/kw_trace.o
$HIPCC --offload-arch=gfx950 $T/kw_bench.o $OBJS $T/kw_trace.o -o tools/kw_bench_trace
$HIPCC -O3 --offload-arch=gfx950 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -DAPRIL_GEMM_TRACE -DAPRIL_KW_ABLATE -I$C -c $C/kernels_gemm_kw.hip -o $T/kw_ablate.o
$HIPCC --offload-arch=gfx950 $T/kw_bench.o $OBJS $T/kw_ablate.o -o tools/kw_bench_ablate
echo built
