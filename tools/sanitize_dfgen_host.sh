#!/bin/bash
# The coefficient generator's host code -- the table writer and readers (host_io.cpp) and the argument checks of is3d_df_generate
# (cf_dfgen.hip, host side) -- under AddressSanitizer + UBSan in a stand-alone program (tools/dfgen_host_check.cpp): no Python, nothing
# preloaded, no GPU needed.  The device code is compiled as usual and never launched without a device.  Leaves the in-tree library alone.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
C="$R/is3d_amd/csrc"
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$C/host_io.cpp" -o "$T/host_io.o"
$HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer -c "$C/cf_dfgen.hip" -o "$T/cf_dfgen.o"
$HIPCC -O1 -g -std=c++17 $SAN -x c++ -c "$R/tools/dfgen_host_check.cpp" -o "$T/check.o"
$HIPCC --offload-arch=gfx950 $SAN -pthread -o "$T/dfgen_host_check" "$T/check.o" "$T/host_io.o" "$T/cf_dfgen.o" -ldl
mkdir "$T/scratch"
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 "$T/dfgen_host_check" "$T/scratch"
