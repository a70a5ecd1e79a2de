#!/bin/bash
# developer experiment: what the fused route's parts cost at Q4_0 4096^3 (gemm_qmx.hip GGML_MX_FUSE_DBG; in every variant the head launch writes the
# whole image, so "mul_mat" = INIT + the variant's product launch and "two" = INIT + the plain launch: the difference is the variant's cost)
#   map_sc1   no quantize in the launch: whole panels per XCD + sc1 image fetches
#   sc1       no quantize, the plain 2 x 4 tile map, sc1 fetches
#   plain     no quantize, plain map, plain fetches (the plain kernel again: the zero of the scale)
#   inject    every workgroup writes its own shares, nothing published or checked; XCD-local map, sc1
#   inject_2x4   the same on the plain map
# usage: tools/experiments/ab_fused_cost.sh build   (no GPU needed)   |   tools/experiments/ab_fused_cost.sh run
cd "$(dirname "$0")/../.."
V="map_sc1:1 sc1:3 plain:7 inject:8 inject_2x4:10"
if [ "$1" = build ]; then
  for v in $V; do tools/build_variant.sh fuse_${v%%:*} gemm_qmx.hip "-DGGML_MX_FUSE_DBG=${v##*:}" || exit 1; done
else
  for v in $V; do
    GGML_HIP_LIB=$PWD/ggmlsharp_amd/lib/dbg/libggml_hip_fuse_${v%%:*}.so timeout -k 10 120 python tools/fused_time.py 4096:4096:4096 || exit $?
  done
fi
