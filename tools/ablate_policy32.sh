#!/bin/bash
# Ablation timing of k_act32 (spl_policy32.hip, -DSPL_POL_ABL=<bits>; wrong results by design except
# "full"): build the variants here (BUILD=1: csrc/Makefile's variant rule through tools/variants.py,
# spl_policy32.hip recompiled and the product's other objects), or time each under
# rocprofv3 kernel-trace stats on the GPU box.  Bits: 1 tanh = identity, 2 one weight chunk (no ring
# streaming, no per-chunk barrier), 4 A planes read once per tile, 8 no MFMA (a VALU stand-in).
set -o pipefail
D=splendor-gym_amd/ablate
VARIANTS=${VARIANTS:-"full:0 notanh:1 noring:2 noafrd:4 noring_notanh:3 mfma_only:7"}
if [ "${BUILD:-0}" = "1" ]; then
  specs=""
  for v in $VARIANTS; do specs="$specs p32_${v%%:*}=-DSPL_POL_ABL=${v#*:}"; done
  python3 tools/variants.py build $specs only=spl_policy32 "lib=$PWD/$D/lib{name}.so" || exit 1
  exit 0
fi
O=gpurun_out/abl_p32
mkdir -p $O
export TMPDIR=/tmp
for v in $VARIANTS; do
  n=${v%%:*}
  SPLENDOR_AMD_LIB=$PWD/$D/libp32_$n.so timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv \
     -d $O/$n -o run -- python3 tools/bench_policy.py --fused-only --iters 20 > $O/$n.json 2> $O/$n.err || { echo "fail $n"; exit 1; }
  echo "$n $(grep -h 'k_act32' $O/$n/run_kernel_stats.csv | cut -d, -f1-4 | tr '\n' ' ')"
done
