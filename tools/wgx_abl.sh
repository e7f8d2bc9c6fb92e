#!/bin/bash
# Timing-only ablations of conv_wgrad_x3_kernel (wgrad_x3.hip, -DWGX_ABL=<bits>): for each of WGX_LIST, scratch/x/wgx_<bits>/lib.so
# (built by tools/variant.py where it is missing; that needs no GPU, so build before going to the GPU box) and the weight-gradient
# launches of one bf16x3 train step on it (tools/train_prof.py).  The first step that fails or overruns ends the script.
set -e
cd "$(dirname "$0")/.."
source tools/steps.sh
for a in ${WGX_LIST:-0 1 2 4 8 3 7}; do
  lib=scratch/x/wgx_$a/lib.so
  [ -f $lib ] || python tools/variant.py wgx_$a wgrad_x3.hip -DWGX_ABL=$a > /dev/null
  HRNET_HIP_LIB=$PWD/$lib step 60 $OUT/wgx_abl.err python tools/train_prof.py bf16x3 > $OUT/wgx_$a.txt     # three train steps after the start-up: 5 s for bench.py's train step in bf16x3, which this is
  echo "WGX_ABL=$a: $(grep conv_wgrad_bf16x3 $OUT/wgx_$a.txt)"
done
