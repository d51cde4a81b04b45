#!/bin/bash
# Builds spsp_host.cpp with AddressSanitizer + UBSan into a program of its own (CPU only: no device, no Python) and runs the
# windows pass's host functions in it: the counting rule, the expansion as plain loops, the segments and mosaic rows with their
# refusals, the two texts, the word check and the plan.
# usage: tests/tools/windows_asan/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../../.." && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -I"$root/include" \
    "$here/main.cpp" "$root/supersampler_amd/csrc/spsp_host.cpp" -o "$work/windows_asan" -lz -lpthread
ASAN_OPTIONS=detect_leaks=1 "$work/windows_asan"
