#!/bin/sh
# Sorted list of (kernel symbol, size) of the gfx950 code object inside a build of libpepsgpu.so: two builds whose lists are
# equal instantiate the same kernels with the same code size (a host-side refactor must leave the list unchanged).
#   sh scripts/kernel_symbols.sh peps_amd/lib/libpepsgpu.so > tree.txt
set -e
LLVM=${ROCM_PATH:-/opt/rocm}/llvm/bin
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
"$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$tmp/fat.bin" "$1" "$tmp/stripped.so"
"$LLVM/clang-offload-bundler" --unbundle --type=o --input="$tmp/fat.bin" --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output="$tmp/gfx950.co"
"$LLVM/llvm-readelf" -sW "$tmp/gfx950.co" | awk '$4 == "FUNC" && $7 != "UND" { print $8, $3 }' | sort
