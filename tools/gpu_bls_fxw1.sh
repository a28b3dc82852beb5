#!/bin/bash
# The BLS final-exponentiation step program at ONE wave per SIMD (spills to
# AGPRs; lib/ab/bls_fx_w1.so) against the shipped pair kernel: c3bls lines
# interleaved, FETCH / WRITE passes of the variant.
#   bash tools/gpu_bls_fxw1.sh OUT
set -u
out=${1:-gpurun_out/blsfxw1}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
for r in 1 2; do
  for lib in indy-plenum_amd/lib/libplenum_verify.so indy-plenum_amd/lib/ab/bls_fx_w1.so; do
    tag=$(basename $lib .so)
    PLENUM_GPU_LIB=$lib timeout -k 10 300 python bench.py --full --config c3bls --steps 3 --warmup 1 --no-cpu-baseline > "$out/c3bls_${tag}_$r.json" 2> "$out/c3bls_${tag}_$r.err" || exit 1
  done
done && \
for c in FETCH_SIZE WRITE_SIZE; do
  PLENUM_GPU_LIB=indy-plenum_amd/lib/ab/bls_fx_w1.so timeout -s KILL 90 rocprofv3 --pmc $c --output-format csv -d "$out/pmc/$c" -o pmc -- \
    python3 bench.py --full --steps 1 --warmup 0 --n 500000 --no-cpu-baseline --no-e2e --config c3bls > "$out/pmc_$c.log" 2>&1 || exit 1
done && echo done
