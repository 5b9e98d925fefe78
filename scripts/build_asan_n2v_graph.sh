#!/bin/bash
# AddressSanitizer + UBSan run of node2vec's device-free graph set-up (gem_amd/csrc/n2v_graph.hip: prepare_n2v_graph, the renaming of the binary-layout
# unigram table) and of sgns_knobs_from_env (gem_amd/csrc/sgns_plan.hip).  Both units are HIP-free, so they are compiled as plain C++ with
# -fsanitize=address,undefined -- no hipcc, no HIP runtime, no other object of the library -- and linked with a driver of their own
# (scripts/asan/n2v_graph_driver.cpp, `self`: unsorted weighted and unweighted rows, a repeated column, a sink and isolated ids, hub rows, weights that
# differ between rows only, one refusal of every kind, the renaming, the knobs' clamps).  A stand-alone program; runs WITHOUT a GPU:
#
#   scripts/build_asan_n2v_graph.sh       # prints the driver's summary and the number of sanitizer reports (expected: 0)
set -e
cd "$(dirname "$0")/.."
OUT=gem_amd/build/asan_n2v_graph
mkdir -p $OUT
CL=/opt/rocm/lib/llvm/bin/clang++
SAN="-fsanitize=address,undefined -fno-omit-frame-pointer"
$CL -x c++ -std=c++17 -O1 -g $SAN -c gem_amd/csrc/n2v_graph.hip -o $OUT/n2v_graph.o
$CL -x c++ -std=c++17 -O1 -g $SAN -c gem_amd/csrc/sgns_plan.hip -o $OUT/sgns_plan.o
$CL -std=c++17 -O1 -g $SAN -c scripts/asan/n2v_graph_driver.cpp -o $OUT/driver.o
$CL $SAN $OUT/driver.o $OUT/n2v_graph.o $OUT/sgns_plan.o -o $OUT/n2v_graph_asan
ASAN_OPTIONS="halt_on_error=0" UBSAN_OPTIONS="print_stacktrace=1" timeout 300 $OUT/n2v_graph_asan self 2> $OUT/err.txt \
    || { tail -30 $OUT/err.txt; echo "driver failed"; exit 1; }
tail -1 $OUT/err.txt
echo "sanitizer reports: $(grep -c 'ERROR: AddressSanitizer\|runtime error:' $OUT/err.txt || true)"
