#!/bin/bash
# A/B of k_act32 build variants (spl_policy32.hip), alternating on one box:
#   BUILD=1 tools/ab_policy32.sh            # here: the variants below into splendor-gym_amd/ablate/
#   tools/ab_policy32.sh [rounds]           # GPU box: tools/bench_policy.py per variant, `rounds` passes
# Variants: name:REV:FLAGS (REV = a git revision of the sources, or "wt" for the working tree; FLAGS, comma
# separated, are added to the product's).  BUILD=1 is csrc/Makefile's variant rule through tools/variants.py:
# spl_policy32.hip (REV's, with REV's headers) recompiled, the other objects the product's own.
set -o pipefail
D=splendor-gym_amd/ablate
VARIANTS=${VARIANTS:-"head:HEAD: wt:wt:"}
if [ "${BUILD:-0}" = "1" ]; then
  specs=""
  for v in $VARIANTS; do
    IFS=: read -r name rev extra <<< "$v"
    [ "$rev" = "wt" ] && rev="" || rev="@$rev"
    specs="$specs p32v_$name$rev=$extra"
  done
  python3 tools/variants.py build $specs only=spl_policy32 "lib=$PWD/$D/lib{name}.so" || exit 1
  exit 0
fi
O=gpurun_out/ab_p32
mkdir -p $O
for r in $(seq 1 ${1:-2}); do
  for v in $VARIANTS; do
    name=${v%%:*}
    SPLENDOR_AMD_LIB=$PWD/$D/libp32v_$name.so timeout -k 10 120 python3 tools/bench_policy.py --fused-only --iters 30 \
      > $O/${name}_$r.json 2> $O/${name}_$r.err || { echo "fail $name"; tail -5 $O/${name}_$r.err; exit 1; }
    echo "$name pass $r $(python3 -c "import json,sys; d=json.load(open('$O/${name}_$r.json')); print(d['fused_fp32_sample_us'], d['fused_fp32_greedy_us'])")"
  done
done
