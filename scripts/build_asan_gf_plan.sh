#!/bin/bash
# AddressSanitizer + UBSan run of GF's host planning (gem_amd/csrc/gf_plan.hip: the acceptance rule, the row plan, the unit schedule and plan, the
# launches of a unit sweep, the rows-per-wavefront rule).  gf_plan.hip is HIP-free, so it is compiled as plain C++ with -fsanitize=address,undefined
# -- no hipcc, no HIP runtime, no other object of the library -- and linked with a driver of its own (scripts/asan/gf_plan_driver.cpp: edge lists
# generated from seeds, one digest line per plan; its output is tests/golden/gf_plan_digest.txt).  A stand-alone program; runs WITHOUT a GPU:
#
#   scripts/build_asan_gf_plan.sh    # prints the number of sanitizer reports (expected: 0) and whether the digests equal the golden
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_gf_plan
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$CL -x c++ -std=c++17 -O1 -g $SAN -c gem_amd/csrc/gf_plan.hip -o $OUT/gf_plan.o
$CL -std=c++17 -O1 -g $SAN -c scripts/asan/gf_plan_driver.cpp -o $OUT/driver.o
$CL $SAN $OUT/driver.o $OUT/gf_plan.o -o $OUT/gf_plan_asan
ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" timeout 900 $OUT/gf_plan_asan digest > $OUT/digest.txt 2> $OUT/err.txt \
    || { tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|runtime error:' $OUT/err.txt || true)"
cmp $OUT/digest.txt tests/golden/gf_plan_digest.txt && echo "digests equal tests/golden/gf_plan_digest.txt ($(wc -l < $OUT/digest.txt) lines)"
