#!/bin/bash
# Ablation timing of k_act (spl_policy.hip, -DSPL_ACT_ABL=<bits>): build variants here
# (BUILD=1), or time each under rocprofv3 kernel-trace stats on the GPU box.
set -o pipefail
D=splendor-gym_amd/ablate
C=splendor-gym_amd/csrc
VARIANTS="full:0 no_mfma:1 no_epi:2 no_xload:4 no_ring:8 only_ring:7 only_mfma:14"
flags_of() { make -s -C $C flags-$1; }  # the flags csrc/Makefile compiles that source with
if [ "${BUILD:-0}" = "1" ]; then
  mkdir -p $D/obj
  others=""
  for s in $(make -s -C $C names); do
    [ $s = spl_policy ] && continue
    others="$others $D/obj/$s.o"
    [ $D/obj/$s.o -nt $C/$s.hip ] || /opt/rocm/bin/hipcc $(flags_of $s) -c -o $D/obj/$s.o $C/$s.hip || exit 1
  done
  for v in $VARIANTS; do
    /opt/rocm/bin/hipcc $(flags_of spl_policy) -DSPL_ACT_ABL=${v#*:} -c -o $D/obj/pol_${v%%:*}.o $C/spl_policy.hip || exit 1
    /opt/rocm/bin/hipcc $(flags_of spl_engine) -shared -o $D/libpol_${v%%:*}.so $others $D/obj/pol_${v%%:*}.o || exit 1
  done
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
