#!/bin/bash
# tools/v6_abl.sh BITS...: timing-only ablation builds of conv3x3_v6.hip (-DV6_ABL=BITS, see the kernel's header), one call of
# tools/variant.py each -> scratch/x/v6_BITS/lib.so; on the GPU box: HRNET_HIP_LIB=scratch/x/v6_BITS/lib.so python tools/kbench.py bf16
set -e
for bits in "$@"; do
  python "$(dirname "$0")/variant.py" v6_$bits conv3x3_v6.hip -DV6_ABL=$bits
done
