#!/bin/bash
# AddressSanitizer + UBSan run of the host arithmetic of HOPE / Laplacian Eigenmaps / LLE (gem_amd/csrc/hope_host.hip: the fp64 small-matrix steps,
# the scheduling rules of the two solvers, the choice of the k outputs, the CSR set-up).  hope_host.hip and sym_eig.hip are HIP-free, so they are
# compiled as plain C++ with -fsanitize=address,undefined -- no hipcc, no HIP runtime, no other object of the library -- and linked with a driver of
# their own (scripts/asan/hope_host_driver.cpp, `self`: inputs generated from seeds, the degenerate ones included).  A stand-alone program; runs
# WITHOUT a GPU:
#
#   scripts/build_asan_hope_host.sh    # prints the driver's failed checks and the number of sanitizer reports (expected: 0 and 0)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_hope_host
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
for f in hope_host sym_eig; do $CL -x c++ -std=c++17 -O1 -g -Wall $SAN -c gem_amd/csrc/$f.hip -o $OUT/$f.o; done
$CL -std=c++17 -O1 -g -Wall $SAN -c scripts/asan/hope_host_driver.cpp -o $OUT/driver.o
$CL $SAN $OUT/driver.o $OUT/hope_host.o $OUT/sym_eig.o -lpthread -o $OUT/hope_host_asan
ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" timeout 900 $OUT/hope_host_asan self > $OUT/self.txt 2> $OUT/err.txt \
    || { grep FAILED $OUT/self.txt || true; tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
tail -1 $OUT/self.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|runtime error:' $OUT/err.txt || true)"
