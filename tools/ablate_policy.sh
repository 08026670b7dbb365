#!/bin/bash
# Ablation timing of k_act (spl_policy.hip, -DSPL_ACT_ABL=<bits>): build variants here (BUILD=1:
# csrc/Makefile's variant rule through tools/variants.py, spl_policy.hip recompiled and the product's other
# objects), or time each under rocprofv3 kernel-trace stats on the GPU box.
set -o pipefail
D=splendor-gym_amd/ablate
VARIANTS=${VARIANTS:-"full:0 no_mfma:1 no_epi:2 no_xload:4 no_ring:8 only_ring:7 only_mfma:14"}
if [ "${BUILD:-0}" = "1" ]; then
  specs=""
  for v in $VARIANTS; do specs="$specs pol_${v%%:*}=-DSPL_ACT_ABL=${v#*:}"; done
  python3 tools/variants.py build $specs only=spl_policy "lib=$PWD/$D/lib{name}.so" || exit 1
  exit 0
fi
O=gpurun_out/abl_pol
mkdir -p $O
export TMPDIR=/tmp
for v in $VARIANTS; do
  n=${v%%:*}
  SPLENDOR_AMD_LIB=$PWD/$D/libpol_$n.so timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv \
     -d $O/$n -o run -- python3 tools/bench_policy.py --fused-only --iters 20 > $O/$n.json 2> $O/$n.err || { echo "fail $n"; exit 1; }
  echo "$n $(grep -h 'k_act' $O/$n/run_kernel_stats.csv | tr '\n' ' ')"
done
