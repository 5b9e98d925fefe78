#!/bin/bash
# AddressSanitizer run of the HOST part of the evaluator handle (gem_amd/csrc/eval.hip: host copies, error paths of gemhip_eval_create /
# _ap / _pairs / _destroy; gem_amd/csrc/eval_host.hip: its device-free arithmetic, called directly) as a stand-alone program with its own main
# (scripts/asan/eval_driver.cpp), in the manner of build_asan_plan.sh.  eval.hip and runtime.hip (the error state) are compiled with the sanitizer on
# the host side only (-Xarch_host; device code as usual), eval_host.hip as plain C++, and linked with the driver.
# Runs WITHOUT a GPU: a well-formed create then stops at its first HIP call and must free what it copied.
# Then tests/test_eval_host.py runs with its driver program (scripts/asan/eval_host_driver.cpp, plain C++) built with AddressSanitizer and UBSan:
# the tests' own inputs go through the sanitized program, nothing sanitized is loaded into python.
#
#   scripts/build_asan_eval.sh       # prints the drivers' summaries and the number of sanitizer reports (expected: 0)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_eval
mkdir -p $OUT
HIPCC=/opt/rocm/bin/hipcc
SAN="-Xarch_host -fsanitize=address -Xarch_host -fno-omit-frame-pointer"
for f in eval runtime; do
    $HIPCC --offload-arch=gfx950 -O1 -g -std=c++17 $SAN -w -c gem_amd/csrc/$f.hip -o $OUT/$f.o &
done
CL=/opt/rocm/lib/llvm/bin/clang++
$CL -x c++ -O1 -g -std=c++17 -fsanitize=address -fno-omit-frame-pointer -c gem_amd/csrc/eval_host.hip -o $OUT/eval_host.o
$HIPCC -x c++ -O1 -g -std=c++17 -fsanitize=address -fno-omit-frame-pointer -c scripts/asan/eval_driver.cpp -o $OUT/driver.o
$CL -x c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-omit-frame-pointer gem_amd/csrc/eval_host.hip scripts/asan/eval_host_driver.cpp -o $OUT/eval_host_asan
wait
$HIPCC --offload-arch=gfx950 -fsanitize=address $OUT/driver.o $OUT/eval.o $OUT/eval_host.o $OUT/runtime.o -o $OUT/eval_asan
ASAN_OPTIONS="halt_on_error=0" timeout 300 $OUT/eval_asan > $OUT/out.txt 2> $OUT/err.txt || { cat $OUT/out.txt; tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
cat $OUT/out.txt
EVAL_HOST_DRIVER=$PWD/$OUT/eval_host_asan ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1" timeout 300 python -m pytest -q -s tests/test_eval_host.py \
    > $OUT/pytest.txt 2>> $OUT/err.txt || { tail -30 $OUT/pytest.txt; echo "tests/test_eval_host.py failed through the sanitized driver"; exit 1; }
tail -1 $OUT/pytest.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|ERROR: LeakSanitizer\|runtime error:' $OUT/err.txt $OUT/pytest.txt | awk -F: '{s += $2} END {print s}')"
