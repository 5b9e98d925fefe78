#!/bin/bash
# AddressSanitizer + UBSan run of the evaluation units' shared ingest checks (gem_amd/csrc/matrix_host.hip: the entry scan, the padded copy,
# the index and pair scans) as a stand-alone program with its own main (scripts/asan/matrix_host_driver.cpp), in the manner of
# build_asan_kmeans.sh.  Plain C++, no HIP, runs on a CPU; nothing sanitized is loaded into python and nothing runs on a GPU.
#
#   scripts/build_asan_matrix_host.sh       # prints the driver's summary and the number of sanitizer reports (expected: 0)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_matrix_host
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
$CL -x c++ -O1 -g -std=c++17 -Wall -fsanitize=address,undefined -fno-omit-frame-pointer gem_amd/csrc/matrix_host.hip scripts/asan/matrix_host_driver.cpp -o $OUT/matrix_host_asan
ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" timeout 300 $OUT/matrix_host_asan > $OUT/out.txt 2> $OUT/err.txt || { cat $OUT/out.txt; tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
cat $OUT/out.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|ERROR: LeakSanitizer\|runtime error:' $OUT/err.txt || true)"
