"""GPU tier of the ranking metrics and link classification (tests/README_link_auc.md): the device sort against numpy's stable argsort, the
metrics against exact rationals, the curve points, the pair features bit for bit, the fused scores, the fit against the exact minimiser, the
protocol end to end against the sklearn fixture, determinism and the refusals.  Nothing here provokes a fault: every refusal is decided on
the host before a launch."""
import ctypes as C
import json

import numpy as np
import pytest

import nc_refs as NR
import rank_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import link_classification as LC
from gem_amd.evaluation import ranking as RK

pytestmark = pytest.mark.gpu

W = 4096                         # keys per sort workgroup (gemhip_rank_info[0]): the row counts below straddle it
PAIRS_PER_WAVE = 8               # pairs a wave has in flight (gemhip_edgeclf_info[2]); 32 per workgroup
B_MFMA = 4 * 1.5e-7              # tests/test_node_classification_gpu.py: the f32 matrix units' error on the Hessian's and gradient's terms
ULP = 2.0 ** -52


@pytest.fixture(scope='module')
def fixture():
    return json.load(open(golden_path('link_auc_ref.json'))), np.load(golden_path('link_auc_ref.npz'))


def test_kernel_constants_are_the_ones_the_shapes_below_were_chosen_for():
    assert RK.sort_info()['keys_per_workgroup'] == W and RK.sort_info()['radix_bits'] == 8
    with LC.EdgeClassifier(np.zeros((2, 1), np.float32)) as ec:
        st = ec.stats()
    assert (st['pairs_per_wave'], st['pairs_per_workgroup']) == (PAIRS_PER_WAVE, 32)


# ------------------------------------------------------------------ sort
def check_sort(s, passes=None):
    s = np.asarray(s, dtype=np.float64)
    perm = RK.argsort_desc(s)
    info = RK.sort_info()
    assert np.array_equal(perm, R.argsort_ref(s))
    assert info['m'] == len(s) and info['passes'] + info['passes_skipped'] == 8 and info['workgroups'] == (len(s) + W - 1) // W
    if passes is not None:
        assert info['passes'] == passes
    return info


@pytest.mark.parametrize('m', [1, 2, W - 1, W, W + 1, 3 * W + 17, (1 << 17) + 3])
def test_sort_every_row_count(m):
    rng = np.random.RandomState(m % 1000)
    check_sort(rng.standard_normal(m))
    check_sort(np.round(rng.standard_normal(m) * 4) / 4)             # heavy ties: stability decides most of the order


def from_bits(bits):
    return np.asarray(bits, dtype=np.uint64).view(np.float64)


def test_sort_special_keys():
    rng = np.random.RandomState(1)
    m = 2 * W + 129
    check_sort(np.full(m, 3.25), passes=0)                             # all equal: every pass skipped, the identity
    check_sort(rng.choice([1.5, -2.0], size=m))
    check_sort(rng.choice([0.0, -0.0], size=m), passes=0)              # one tie group, the original order
    check_sort(rng.choice([0.0, -0.0, 1.0, -1.0], size=m))
    check_sort(rng.choice([np.inf, -np.inf, 0.0, 1e308, -1e308], size=m))
    check_sort(from_bits(rng.randint(0, 1 << 20, size=m)) * rng.choice([1.0, -1.0], size=m))          # denormals of both signs
    check_sort(-np.abs(rng.standard_normal(m)))
    check_sort(from_bits(0x3FF0000000000000 + rng.randint(0, 256, size=m)), passes=1)                 # only the lowest byte differs
    check_sort(from_bits((rng.randint(0, 128, size=m).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0010000000000000)), passes=1)      # only the highest
    check_sort(from_bits((rng.randint(0, 256, size=m).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0010000000000000)))                # ... of both signs


def test_sort_refusals_and_limits():
    L = _hip.lib()
    s = np.array([1.0, np.nan]); perm = np.zeros(2, np.int32)
    assert L.gemhip_rank_argsort(2, _hip.ptr(s, C.c_double), _hip.ptr(perm, C.c_int32)) == _hip.E_INVALID
    assert L.gemhip_last_error() == b'rank_argsort: score[1] is NaN'
    assert L.gemhip_rank_argsort(1 << 31, _hip.ptr(s, C.c_double), _hip.ptr(perm, C.c_int32)) == _hip.E_UNSUPPORTED


# ------------------------------------------------------------------ metrics
@pytest.fixture(scope='module')
def metric_cases():
    sets = R.metric_sets()
    sets['curve'] = R.curve_set()
    return {name: (s, y, R.exact_scores(s, y)) for name, (s, y) in sets.items()}


@pytest.mark.parametrize('name', ['continuous', 'quantised_8', 'quantised_64', 'separated_up', 'separated_down', 'all_tied', 'one_positive_first',
                                  'one_positive_last', 'curve'])
def test_metrics_against_the_exact_rationals(name, metric_cases):
    s, y, ex = metric_cases[name]
    got = RK.binary_ranking_scores(s, y)
    auc, ap = float(ex['auc']), float(ex['ap'])
    print('%s: auc %.17g (exact %.17g)  ap %.17g (exact %.17g, bound %.2e)  T %d  kernel %.3f ms' %
          (name, got['auc'], auc, got['ap'], ap, 4 * ex['T'] * 2.0 ** -53 * ap, ex['T'], got['kernel_ms']))
    assert (got['n_pos'], got['n_neg'], got['n_thresholds'], got['u2']) == (ex['P'], ex['N'], ex['T'], ex['U2'])
    assert abs(got['auc'] - auc) <= ULP * auc
    assert abs(got['ap'] - ap) <= 4 * ex['T'] * 2.0 ** -53 * ap
    assert got['prevalence'] == ex['P'] / float(len(s))
    thr, tp, fp = RK.group_table(s, y)
    assert np.array_equal(thr, ex['thr']) and np.array_equal(tp, ex['tp']) and np.array_equal(fp, ex['fp'])
    if name == 'separated_up':
        assert got['auc'] == 1.0 and got['ap'] == 1.0
    if name in ('separated_down', 'one_positive_last'):
        assert got['auc'] == 0.0
    if name == 'all_tied':
        assert got['auc'] == 0.5 and got['n_thresholds'] == 1 and abs(got['ap'] - got['prevalence']) <= ULP


def test_curves_against_the_sklearn_fixture(fixture):
    meta, arr = fixture
    s, y = R.curve_set()
    tol = 4 * meta['curve']['sklearn_vs_exact']
    fpr, tpr, thr = RK.roc_curve(s, y)
    prec, rec, pthr = RK.precision_recall_curve(s, y)
    for got, key in ((fpr, 'roc_fpr'), (tpr, 'roc_tpr'), (prec, 'pr_precision'), (rec, 'pr_recall')):
        assert got.shape == arr[key].shape and np.all(np.abs(got - arr[key]) <= tol), key
    assert np.array_equal(thr, arr['roc_thr']) and np.array_equal(pthr, arr['pr_thr'])


def test_curve_refuses_too_small_a_buffer_and_reports_T():
    L = _hip.lib()
    s, y = R.curve_set()
    s = np.ascontiguousarray(s); y = np.ascontiguousarray(y, dtype=np.uint8)
    T = C.c_int64(-1)
    rc = L.gemhip_rank_curve(len(s), _hip.ptr(s, C.c_double), _hip.ptr(y, C.c_uint8), 10, None, None, None, C.byref(T))
    assert rc == _hip.E_INVALID and T.value == len(np.unique(s))
    assert L.gemhip_last_error() == b'rank_curve: %d distinct scores, room for 10' % T.value


# ------------------------------------------------------------------ pair features and fused scores
def padded(X, extra=3):
    out = np.full((X.shape[0], X.shape[1] + extra), np.nan, np.float32)          # the device must never read the padding
    out[:, :X.shape[1]] = X
    return out


def pair_list(rng, n, m):
    st = rng.randint(0, n, size=m).astype(np.int32); ed = rng.randint(0, n, size=m).astype(np.int32)
    if m > 2:
        ed[1] = st[1]                                                    # a pair with itself
        st[-1], ed[-1] = st[0], ed[0]                                    # a repeated pair
    return st, ed


@pytest.mark.parametrize('d', [1, 2, 32, 33, 128, 255])
def test_features_and_scores_every_width_and_pair_count(d):
    rng = np.random.RandomState(200 + d)
    n = 300
    X = rng.standard_normal((n, d)).astype(np.float32)
    with LC.EdgeClassifier(padded(X), d=d) as ec:
        for m in (1, 63, 64, 65, 1061):
            st, ed = pair_list(rng, n, m)
            w = rng.standard_normal(d + 1)
            for op in R.OPS:
                F = ec.features(op, st, ed)
                assert F.dtype == np.float32 and np.array_equal(F, R.features_ref(op, X, st, ed)), (op, m)
                z = ec.decision_function(op, st, ed, w)
                err = np.abs(z - R.scores_ref(F, w)) / R.score_bound(F, w)
                assert err.max() <= 1.0, (op, m, err.max())
            A, B = X[st].astype(np.float64), X[ed].astype(np.float64)
            bound = 4 * (d + 1) * 2.0 ** -53 * (np.abs(A) * np.abs(B)).sum(1)
            assert np.all(np.abs(ec.dot(st, ed) - (A * B).sum(1)) <= bound), m


def test_operators_at_the_edges_of_float32():
    X = np.array([[1e18, -1e18, 1e-30, 0.0], [1e18, 1e18, -1e-30, -0.0], [3.0000002, 1.0000001, 1e-45, 7.0]], np.float32)
    st = np.array([0, 0, 1, 2, 2], np.int32); ed = np.array([1, 2, 2, 0, 2], np.int32)
    with LC.EdgeClassifier(X) as ec:
        for op in R.OPS:
            F = ec.features(op, st, ed)
            assert np.array_equal(F, R.features_ref(op, X, st, ed)) and np.all(np.isfinite(F)), op


# ------------------------------------------------------------------ the fit, and the protocol end to end
@pytest.fixture(scope='module')
def split():
    train, test, pairs = R.fixture_pairs()
    return train, test, pairs, R.embedding()


@pytest.fixture(scope='module')
def fits(split):
    """One device fit per operator on the fixture's training pairs, shared by the tests below."""
    _, _, pairs, X = split
    with LC.EdgeClassifier(X) as ec:
        return {op: ec.fit(op, *pairs['train']) for op in R.OPS}


@pytest.mark.parametrize('op', R.OPS)
def test_fit_against_the_exact_minimiser(op, split, fits, fixture):
    _, _, pairs, X = split
    st, ed, y = pairs['train']
    wstar = fixture[1]['w_' + op]
    w, info = fits[op]
    F = R.features_ref(op, X, st, ed)
    scale = np.abs(wstar).max()
    w32 = np.asarray(NR.newton_fit(F, y, 1.0, None, np.float32)[0], np.float64)
    dev32 = np.abs(w32 - wstar).max() / scale
    Xa = NR.augment(F, np.float64)
    _, _, H = NR.pass_ref(Xa, y, wstar, 1.0)
    p, q, _ = NR.sigma_parts(Xa @ wstar)
    dg = B_MFMA * (np.abs(Xa).T @ np.where(y > 0, q, p)).max()
    derived = np.abs(np.linalg.inv(H)).sum(1).max() * dg / scale
    dev = np.abs(w - wstar).max() / scale
    print('%s: device %.3e   4 x float32 restatement %.3e   derived %.3e   iterations %d backtracks %d passes %d' %
          (op, dev, 4 * dev32, derived, info['iterations'], info['backtracks'], info['passes']))
    assert dev <= max(4 * dev32, derived)
    assert info['converged'] and info['degenerate'] == 0 and info['iterations'] >= 1 and info['passes'] == info['iterations']


@pytest.mark.parametrize('op', R.OPS + ('dot', 'method'))
def test_protocol_end_to_end_against_the_fixture(op, split, fixture):
    train, test, pairs, X = split
    meta = fixture[0]
    entry = meta['ops']['dot' if op == 'method' else op]

    class InnerProduct(object):                                          # a method whose edge weight is X[i] . X[j], as GF's and node2vec's
        def get_method_name(self):
            return 'graph_factor_sgd'
    res = LC.evaluate_link_classification(train, test, X, op=op, seed=R.PAIR_SEED, graph_embedding=InnerProduct() if op == 'method' else None)
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        assert res[k] == meta[k]
    P, N = res['n_test_pos'], res['n_test_neg']
    auc_bound = entry['near'] / float(P * N) + ULP
    ap_bound = entry['ap_sensitivity'] + 4 * entry['n_thresholds'] * 2.0 ** -53
    print('%s: auc %.12f (fixture %.12f, |diff| %.2e, bound %.2e)  ap %.12f (fixture %.12f, |diff| %.2e, bound %.2e)  fit %.3f s  score %.3f s  rank %.3f s' %
          (op, res['auc'], entry['auc'], abs(res['auc'] - entry['auc']), auc_bound, res['ap'], entry['ap'], abs(res['ap'] - entry['ap']), ap_bound,
           res['fit_s'], res['score_s'], res['rank_s']))
    assert entry['near_share'] <= 1e-3
    assert abs(res['auc'] - entry['auc']) <= auc_bound
    assert abs(res['ap'] - entry['ap']) <= ap_bound
    assert (res['coef'] is None) == (op in ('dot', 'method'))


def test_two_runs_give_identical_bytes(split, fits):
    _, _, pairs, X = split
    rng = np.random.RandomState(9)
    s = np.round(rng.standard_normal(3 * W + 17) * 16) / 16
    y = (rng.random_sample(len(s)) < 0.5).astype(np.uint8)
    assert np.array_equal(RK.argsort_desc(s), RK.argsort_desc(s))
    a, b = RK.binary_ranking_scores(s, y), RK.binary_ranking_scores(s, y)
    assert all(a[k] == b[k] for k in a if k != 'kernel_ms')
    with LC.EdgeClassifier(X) as ec:
        for op in ('hadamard', 'l2'):
            w, _ = ec.fit(op, *pairs['train'])
            assert np.array_equal(w, fits[op][0])
            st, ed, _ = pairs['test']
            assert np.array_equal(ec.decision_function(op, st, ed, w), ec.decision_function(op, st, ed, w))


def test_pair_refusals_name_the_position():
    L = _hip.lib()
    X = np.ones((5, 3), np.float32)
    good = np.array([0, 1, 2], np.int32)
    with LC.EdgeClassifier(X) as ec:
        for st, ed, words in ((np.array([0, 5, 1], np.int32), good, 'pair 1 = (5,1) outside [0,5)'), (good, np.array([0, 1, -1], np.int32), 'pair 2 = (2,-1) outside [0,5)')):
            for call in (lambda: ec.features('l1', st, ed), lambda: ec.dot(st, ed), lambda: ec.decision_function('l1', st, ed, np.zeros(4)),
                         lambda: ec.fit('l1', st, ed, [0, 1, 0])):
                with pytest.raises(_hip.GemHipError, match='error -1') as e:
                    call()
                assert words in str(e.value)
        for op in (-1, 4):
            with pytest.raises(_hip.GemHipError, match=r'operator %d outside \[0,4\)' % op):
                ec.features(op, good, good)
        with pytest.raises(_hip.GemHipError, match='m = 0 pairs'):
            ec.features('average', good[:0], good[:0])
        with pytest.raises(_hip.GemHipError, match=r'label\[2\] = 2 is neither 0 nor 1'):
            ec.fit('average', good, good, [0, 1, 2])
        with pytest.raises(_hip.GemHipError, match=r'w\[1\] is not finite'):
            ec.decision_function('average', good, good, [0.0, np.inf, 0.0, 0.0])
        with pytest.raises(_hip.GemHipError, match='C = 0'):
            ec.fit('average', good, good, [0, 1, 0], C=0.0)
        w, info = ec.fit('average', good, good, [1, 1, 1], warn=False)                     # one class only: the solver's degenerate answer, flagged
        assert info['degenerate'] == 1 and w[-1] == np.inf and not w[:-1].any()
    assert L.gemhip_edgeclf_features(None, 0, 1, _hip.ptr(good, C.c_int32), _hip.ptr(good, C.c_int32), None) == _hip.E_INVALID
