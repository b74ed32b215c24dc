#!/bin/bash
# The host entries of the HBT correlation functions -- is3d_hbt_list, is3d_hbt_radii, is3d_write_hbt (hbt_host.cpp, through the rule of
# cf_sampler_hbt.h) -- and their refusals under AddressSanitizer + UBSan in a stand-alone program (tools/hbt_host_check.cpp): no Python,
# nothing preloaded, no GPU needed.  host_io.cpp comes along for the error string.  Leaves the in-tree library alone.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
C="$R/is3d_amd/csrc"
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$C/host_io.cpp" -o "$T/host_io.o"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$C/hbt_host.cpp" -o "$T/hbt_host.o"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$R/tools/hbt_host_check.cpp" -o "$T/check.o"
$HIPCC $SAN -pthread -o "$T/hbt_host_check" "$T/check.o" "$T/hbt_host.o" "$T/host_io.o" -ldl
mkdir "$T/scratch"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$T/hbt_host_check" "$T/scratch"
