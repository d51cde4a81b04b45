#!/bin/bash
# Builds spsp_host.cpp with AddressSanitizer + UBSan into a program of its own (CPU only: no device, no Python) and runs the
# extraction's host functions in it: the records' starts, the extraction, the two flag functions with their refusals and the plan.
# usage: tests/tools/extract_asan/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../../.." && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -I"$root/include" \
    "$here/main.cpp" "$root/supersampler_amd/csrc/spsp_host.cpp" -o "$work/extract_asan" -lz -lpthread
ASAN_OPTIONS=detect_leaks=1 "$work/extract_asan"
