#!/bin/bash
# AddressSanitizer + UBSan run of the schedules of the N-GPU entry points (gem_amd/csrc/multi_plan.hip: the balanced split, GF's row blocks and the
# shardable-order rule, node2vec's shards / episode table / alpha bookkeeping, cut and paste of a table partition).  The unit is HIP-free, so it is
# compiled as plain C++ with -fsanitize=address,undefined -- no hipcc, no HIP runtime, no other object of the library -- and linked with a driver of its
# own (scripts/asan/multi_plan_driver.cpp, `self`: empty shards and empty episode slices, a total divisible by ranks x episodes, n < ranks, ranks that
# own no row, every refusal of the GF rule, 200 random edge lists).  A stand-alone program; runs WITHOUT a GPU:
#
#   scripts/build_asan_multi_plan.sh      # prints the driver's summary and the number of sanitizer reports (expected: 0)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_multi_plan
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$CL -x c++ -std=c++17 -O1 -g $SAN -c gem_amd/csrc/multi_plan.hip -o $OUT/multi_plan.o
$CL -std=c++17 -O1 -g $SAN -c scripts/asan/multi_plan_driver.cpp -o $OUT/driver.o
$CL $SAN $OUT/driver.o $OUT/multi_plan.o -o $OUT/multi_plan_asan
ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" timeout 300 $OUT/multi_plan_asan self 2> $OUT/err.txt \
    || { tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
tail -1 $OUT/err.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|runtime error:' $OUT/err.txt || true)"
