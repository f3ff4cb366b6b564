#!/bin/bash
# VGPRs, scratch bytes per lane and waves per SIMD of every kernel of one csrc/*.hip file, one sorted line each, from
# hipcc's kernel-resource-usage remarks (compiles for gfx950 on a machine without a GPU).  Run it on the parent commit and on
# the tree and diff the two outputs: a kernel that changed shows as a changed line, a new kernel as an added one.
#   tools/dev/kernel_resources.sh gemm_pc.hip > after.txt
set -euo pipefail
cd "$(dirname "$0")/../../graph_odenet_amd/csrc"
obj=$(mktemp --suffix=.o)
trap 'rm -f "$obj"' EXIT
${HIPCC:-/opt/rocm/bin/hipcc} -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function -I../../include \
    -Rpass-analysis=kernel-resource-usage -c "$1" -o "$obj" 2>&1 \
  | grep -E "Function Name|VGPRs:|ScratchSize|Occupancy" | paste - - - - \
  | sed -E 's/.*Function Name: ([^ ]+).*VGPRs: ([0-9]+).*ScratchSize \[bytes\/lane\]: ([0-9]+).*Occupancy \[waves\/SIMD\]: ([0-9]+).*/\1 \2 \3 \4/' \
  | c++filt | sort
