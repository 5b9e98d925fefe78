"""Runs the evaluation units (k-means, t-SNE, node classification, edge classifier, neighbourhood scores, evaluator) through ctypes on the
fixed seeded inputs of tests/eval_units_refs.py and prints one SHA-256 per output array.  Needs a device.

    python scripts/digest_eval_units.py [--out tests/golden/eval_units_digest.json] [--lib <libgem_hip.so of another checkout>]

The run is made twice; an output whose two digests differ is printed as UNSTABLE and left out of --out (every unit documents "the same bits
on every run", so that is a finding).  tests/test_eval_units_digest_gpu.py compares the built library with the file.  The digests are tied to
the compiler: re-record only on a commit for which scripts/compare_kernel_isa.py reports no difference from the commit that recorded them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
if '--lib' in sys.argv:
    os.environ['GEM_HIP_LIB'] = sys.argv[sys.argv.index('--lib') + 1]          # read by gem_amd._hip on import


def main():
    import eval_units_refs as R
    from gem_amd import _hip
    first, second = R.digests(), R.digests()
    unstable = sorted(k for k in first if first[k] != second[k])
    for k in sorted(first):
        print('%s  %s%s' % (first[k], k, '  UNSTABLE' if k in unstable else ''))
    print('%d outputs from %s, %d unstable' % (len(first), _hip.LIB_PATH, len(unstable)))
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            json.dump({k: v for k, v in first.items() if k not in unstable}, f, indent=1, sort_keys=True)
            f.write('\n')
    return 1 if unstable else 0


if __name__ == '__main__':
    sys.exit(main())
