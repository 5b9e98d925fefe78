#!/bin/bash
# ThreadSanitizer run of the threaded host eigensolver (gem_amd/csrc/sym_eig.hip: eig_reduce_mt's spin barriers, the chunked back-transformation).
# sym_eig.hip is HIP-free, so it is compiled as plain C++ with -fsanitize=thread -- no hipcc, no HIP runtime, no other object of the library -- and
# linked with a small driver of its own (scripts/tsan/eig_driver.cpp, through sym_eig.hpp: dense, diagonal -- every step takes the zero-reflector
# branch -- and half-zero matrices at 2, 3 and 4 threads, partial and full solver).  A stand-alone program; runs WITHOUT a GPU:
#
#   scripts/build_tsan_eig.sh        # prints the driver's lines and the number of ThreadSanitizer reports (expected: 0)
#
# (TSan slows the threads enough that the contended-host bail-out of eig_reduce_mt is taken too, so that path is covered as well.)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/tsan
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
$CL -x c++ -std=c++17 -O1 -g -fsanitize=thread -c gem_amd/csrc/sym_eig.hip -o $OUT/sym_eig.o
$CL -std=c++17 -O1 -g -fsanitize=thread -c scripts/tsan/eig_driver.cpp -o $OUT/driver.o
$CL -fsanitize=thread $OUT/driver.o $OUT/sym_eig.o -o $OUT/eig_tsan
TSAN_OPTIONS="halt_on_error=0" timeout 900 $OUT/eig_tsan > $OUT/out.txt 2>&1 || { tail -30 $OUT/out.txt; echo "driver failed"; exit 1; }
tail -3 $OUT/out.txt
echo "ThreadSanitizer reports: $(grep -c 'WARNING: ThreadSanitizer' $OUT/out.txt || true)"
