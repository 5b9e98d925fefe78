"""CPU test of the evaluation units' device-free ingest checks (gem_amd/csrc/matrix_host.hip: first_bad_entry, pad_rows, first_bad_index,
first_bad_pair) as plain C++ behind scripts/asan/matrix_host_driver.cpp: no HIP, no library, no device.  The driver holds the cases (n = 1,
d = ld and d < ld with NaN in the padding, the first of two offenders, the inclusive magnitude bound, pad_rows at dpad = d and dpad > d,
empty lists, INT32_MIN as an index) and the values worked out by hand; scripts/build_asan_matrix_host.sh runs the same program under
AddressSanitizer and UBSan."""
import os
import subprocess

from gem_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_matrix_host_driver(tmp_path):
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    exe = str(tmp_path / 'matrix_host_driver')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(ROOT, 'gem_amd', 'csrc', 'matrix_host.hip'),
                           os.path.join(ROOT, 'scripts', 'asan', 'matrix_host_driver.cpp'), '-o', exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True)
    assert out.returncode == 0 and out.stdout.strip() == 'matrix_host driver: 0 failure(s)', out.stdout
