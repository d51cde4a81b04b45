#!/bin/bash
# Builds spsp_host.cpp with AddressSanitizer + UBSan into a program of its own (CPU only: no device, no Python) and runs the host
# functions of "raw coordinates" in it: the lift as plain loops on FASTA and FASTQ texts with its refusals, the BED text and the plan.
# usage: tests/tools/lift_asan/run.sh
set -e
here=$(cd "$(dirname "$0")" && pwd); root=$(cd "$here/../../.." && pwd)
work=$(mktemp -d)
trap 'rm -rf "$work"' EXIT
g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
    -D__HIP_PLATFORM_AMD__ -I"${ROCM:-/opt/rocm}/include" -I"$root/include" \
    "$here/main.cpp" "$root/supersampler_amd/csrc/spsp_host.cpp" -o "$work/lift_asan" -lz -lpthread
ASAN_OPTIONS=detect_leaks=1 "$work/lift_asan"
