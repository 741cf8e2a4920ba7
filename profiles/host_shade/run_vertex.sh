#!/bin/bash
# bash profiles/host_shade/run_vertex.sh  — the vertex function (kernels/vertex_simple.hip.h) as host C++ under ASan + UBSan,
# on random first vertices, compared with the seam's mat_scatter (CPU only)
set -e
H=$(cd "$(dirname "$0")" && pwd); K=$H/../../crust-render_amd/csrc/kernels; T=${TMPDIR:-/tmp}/crt_host_vertex; mkdir -p $T
CXX=/opt/rocm/lib/llvm/bin/clang++
F="-std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -I$H -I$K -I$H/../../include -Wno-unused-function -Wno-unknown-attributes"
$CXX $F -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer $H/vertex_host.cpp -o $T/vertex_ubsan
$T/vertex_ubsan
