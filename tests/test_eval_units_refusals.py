"""The create functions of the evaluation units (k-means, node classification, edge classifier, t-SNE and its kNN, neighbourhood scores,
evaluator) refuse what they refused, with the return code and the words tests/golden/eval_units_refusals.txt records from the library before
the units' ingest checks moved into matrix_host.hip and eval_common.hpp (scripts/make_golden_eval_refusals.py).  Every refusal precedes the
unit's first HIP call, so this runs without a GPU; a case the host checks accept is only required to get past them."""
import eval_units_refs as R
from conftest import golden_path


def test_every_create_refuses_as_recorded():
    want = open(golden_path('eval_units_refusals.txt')).read().splitlines()
    cases = R.all_cases()
    assert len(want) == len(cases) > 130
    seen = set()
    for (unit, what, thunk), line in zip(cases, want):
        assert R.record_line(unit, what, *thunk()) == line
        seen.add(unit)
    assert seen == set(R.MATRIX_UNITS) | {'nbr_create', 'eval_create'}


def test_the_record_covers_the_rules():
    """Per matrix unit: the three non-finite values at X[2][1], the last entry, the padding column (accepted), the double fault, and for the
    units with a magnitude bound the bound itself (accepted) and the next float above it (refused)."""
    lines = [line.split('\t') for line in open(golden_path('eval_units_refusals.txt')).read().splitlines()]
    for unit, (max_d, max_abs) in R.MATRIX_UNITS.items():
        mine = {f[1]: f[2:] for f in lines if f[0] == unit}
        for what in ('NaN at X[2][1]', '+inf at X[2][1]', '-inf at X[2][1]'):
            assert mine[what][0] == '-1' and 'X[2][1]' in mine[what][1]
        assert 'X[%d][%d]' % (R.N - 1, R.D - 1) in mine['NaN in the last entry of the last row'][1]
        assert mine['NaN in the padding column X[2][3]'] == [R.ACCEPTED]
        assert 'need 1 <= d <= ld' in mine['ld < d and NULL X'][1] and mine['NULL X'][1].endswith('NULL X')
        if max_d is not None:
            assert mine['d one above the limit'][0] == '-3' and 'at most %d' % max_d in mine['d one above the limit'][1]
        if max_abs is not None:
            assert mine['the magnitude bound itself at X[2][1]'] == [R.ACCEPTED] and mine['the next float above the bound at X[2][1]'][0] == '-1'
