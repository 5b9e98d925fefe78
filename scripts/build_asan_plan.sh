#!/bin/bash
# AddressSanitizer + UBSan run of the SGNS host arithmetic (gem_amd/csrc/sgns_plan.hip: the launch rule, bucket_knobs, the unigram table builder).
# sgns_plan.hip is HIP-free, so it is compiled as plain C++ with -fsanitize=address,undefined -- no hipcc, no HIP runtime, no other object of the
# library -- and linked with a driver of its own (scripts/asan/plan_driver.cpp: the launch-rule grid whose output is tests/golden/sgns_plan_grid.txt,
# then the table builder on small inputs with its invariants).  A stand-alone program; runs WITHOUT a GPU:
#
#   scripts/build_asan_plan.sh       # prints the driver's summary, the number of sanitizer reports (expected: 0) and whether the grid equals the golden
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_plan
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$CL -x c++ -std=c++17 -O1 -g $SAN -c gem_amd/csrc/sgns_plan.hip -o $OUT/sgns_plan.o
$CL -std=c++17 -O1 -g $SAN -c scripts/asan/plan_driver.cpp -o $OUT/driver.o
$CL $SAN $OUT/driver.o $OUT/sgns_plan.o -o $OUT/plan_asan
ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" timeout 900 $OUT/plan_asan grid tests/golden/rmat_token_count_histograms.json > $OUT/grid.txt 2> $OUT/err.txt \
    || { tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
tail -1 $OUT/err.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|runtime error:' $OUT/err.txt || true)"
cmp $OUT/grid.txt tests/golden/sgns_plan_grid.txt && echo "grid equals tests/golden/sgns_plan_grid.txt ($(wc -l < $OUT/grid.txt) cases)"
