"""Writes tests/golden/eval_units_refusals.txt: (return code, gemhip_last_error()) of every refusal case of the evaluation units' create
functions (tests/eval_units_refs.py), one tab-separated line per case, from the library GEM_HIP_LIB names (default: the built one).  The
refusals are decided before the first HIP call: no device needed.  Record it from the library whose wording is the reference, then run
tests/test_eval_units_refusals.py against the library under test.

    GEM_HIP_LIB=<parent checkout>/gem_amd/libgem_hip.so python scripts/make_golden_eval_refusals.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)


def main():
    import eval_units_refs as R
    from gem_amd import _hip
    lines = R.record()
    with open(os.path.join(ROOT, 'tests', 'golden', 'eval_units_refusals.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('%d cases from %s, %d refused' % (len(lines), _hip.LIB_PATH, sum(not l.endswith(R.ACCEPTED) for l in lines)))


if __name__ == '__main__':
    main()
