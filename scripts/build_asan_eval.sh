#!/bin/bash
# AddressSanitizer run of the HOST part of the evaluator handle (gem_amd/csrc/eval.hip: validation, host copies, error paths of gemhip_eval_create /
# _ap / _pairs / _destroy) as a stand-alone program with its own main (scripts/asan/eval_driver.cpp), in the manner of build_asan_plan.sh.  eval.hip and
# runtime.hip (the error state) are compiled with the sanitizer on the host side only (-Xarch_host; device code as usual) and linked with the driver.
# Runs WITHOUT a GPU: a well-formed create then stops at its first HIP call and must free what it copied.
#
#   scripts/build_asan_eval.sh       # prints the driver's summary and the number of sanitizer reports (expected: 0)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_eval
mkdir -p $OUT
HIPCC=/opt/rocm/bin/hipcc
SAN="-Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer"
for f in eval runtime; do
    $HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 $SAN -w -c gem_amd/csrc/$f.hip -o $OUT/$f.o &
done
$HIPCC -x c++ -O1 -g -std=c++17 -fsanitize=address -fno-omit-frame-pointer -c scripts/asan/eval_driver.cpp -o $OUT/driver.o
wait
$HIPCC --offload-arch=gfx950 -fsanitize=address $OUT/driver.o $OUT/eval.o $OUT/runtime.o -o $OUT/eval_asan
ASAN_OPTIONS="halt_on_error=0" timeout 300 $OUT/eval_asan > $OUT/out.txt 2> $OUT/err.txt || { cat $OUT/out.txt; tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
cat $OUT/out.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|ERROR: LeakSanitizer' $OUT/err.txt || true)"
