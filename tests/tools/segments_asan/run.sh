#!/bin/bash
# Builds spsp_host.cpp with AddressSanitizer + UBSan into a program of its own (CPU only: no device, no Python) and runs the host
# functions of "segments as sequence" in it: the smoothing with its refusals, the selection's words and flags, the word check, the
# FASTA text as plain loops and the plan.
# usage: tests/tools/segments_asan/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../../.." && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -I"$root/include" \
    "$here/main.cpp" "$root/supersampler_amd/csrc/spsp_host.cpp" -o "$work/segments_asan" -lz -lpthread
ASAN_OPTIONS=detect_leaks=1 "$work/segments_asan"
