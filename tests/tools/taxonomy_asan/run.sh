#!/bin/bash
# Builds spsp_host.cpp with AddressSanitizer + UBSan into a program of its own (CPU only: no device, no Python) and runs the
# taxonomy's host functions in it: the lineage parser, the tree check, the plan and the two CSV writers with their refusals.
# usage: tests/tools/taxonomy_asan/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../../.." && pwd)
work=$(mktemp -d)
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -I"$root/include" \
    "$here/main.cpp" "$root/supersampler_amd/csrc/spsp_host.cpp" -o "$work/taxonomy_asan" -lz -lpthread
ASAN_OPTIONS=detect_leaks=1 "$work/taxonomy_asan"
rm -rf "$work"
