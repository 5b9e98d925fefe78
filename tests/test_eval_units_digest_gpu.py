"""The evaluation units compute the same bits as before their scaffolding moved into matrix_host.hip and eval_common.hpp: one SHA-256 per
output array of k-means, t-SNE, node classification, the edge classifier, the neighbourhood scores and the evaluator on the fixed seeded
inputs of eval_units_refs.py, against tests/golden/eval_units_digest.json (scripts/digest_eval_units.py, recorded from the library of the
commit before the move; two runs there agreed on every output).

The file is tied to the compiler: another compiler may order the same fp64 sums differently without being wrong.  It is re-recorded only on a
commit for which scripts/compare_kernel_isa.py reports no difference from the commit that recorded it."""
import json

import pytest

import eval_units_refs as R
from conftest import golden_path


@pytest.mark.gpu
def test_outputs_hash_as_recorded():
    want = json.load(open(golden_path('eval_units_digest.json')))
    got = R.digests()
    assert sorted(got) == sorted(want) and len(want) == 83
    for must in ('kmeans.inertia', 'tsne.kl', 'tsne.z'):                   # the outputs of the one sum kernel both units share
        assert all('%s n=%d' % (must, n) in want for n in R.DIGEST_SIZES)
    different = sorted(k for k in want if got[k] != want[k])
    assert not different, different
