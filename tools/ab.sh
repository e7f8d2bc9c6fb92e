#!/bin/bash
# usage (on the GPU box): tools/ab.sh VARIANT...  - A/B timing of kernel variants in ONE call (boxes differ by 3-5 %):
# tools/kbench.py for each variant, twice, round-robin; "prod" = the in-tree library, any other name = scratch/x/NAME/lib.so
# (tools/variant.py builds such libraries).  Prints ms per forward and the average launch of every conv family.
# The first kbench.py that fails or overruns its limit ends the script (tools/steps.sh).
source "$(dirname "$0")/steps.sh"
for rep in 1 2; do
for v in "$@"; do
  if [ "$v" = prod ]; then unset HRNET_HIP_LIB; else export HRNET_HIP_LIB=scratch/x/$v/lib.so; fi
  step 60 $OUT/ab_$v.err python tools/kbench.py bf16 > $OUT/ab_$v.txt       # five forwards after the start-up: 2 s
  f() { grep -E "$1" $OUT/ab_$v.txt | awk '{print $4}'; }
  echo "$v: $(grep 'ms/fwd' $OUT/ab_$v.txt | sed 's/.*: //') | 128x128+res $(f '128x128\+res') | 128x128 $(f '128x128 ') | 128x64+res $(f '128x64\+res') | 64x64 $(f '64x64 ') | 64x64+res $(f '64x64\+res')"
done; done
