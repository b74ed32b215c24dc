#!/bin/bash
# The host entries of the differential flow -- is3d_flow_diff_list, is3d_flow_diff_reference, is3d_flow_diff_cumulants, is3d_write_flow_diff
# (flow_diff_host.cpp, through the rules of cf_sampler_flow.h and cf_sampler_flow_diff.h) -- and their refusals under AddressSanitizer + UBSan
# in a stand-alone program (tools/flow_diff_host_check.cpp): no Python, nothing preloaded, no GPU needed.  flow_host.cpp comes along for the
# checks and cumulants it shares, host_io.cpp for the error string.  Leaves the in-tree library alone.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
C="$R/is3d_amd/csrc"
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$C/host_io.cpp" -o "$T/host_io.o"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$C/flow_host.cpp" -o "$T/flow_host.o"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$C/flow_diff_host.cpp" -o "$T/flow_diff_host.o"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$R/tools/flow_diff_host_check.cpp" -o "$T/check.o"
$HIPCC $SAN -pthread -o "$T/flow_diff_host_check" "$T/check.o" "$T/flow_diff_host.o" "$T/flow_host.o" "$T/host_io.o" -ldl
mkdir "$T/scratch"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$T/flow_diff_host_check" "$T/scratch"
