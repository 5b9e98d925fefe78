"""CPU tier of the ranking metrics and link classification (tests/README_link_auc.md): the restatements against sklearn, the host half
against the exact rationals, the non-edge sampler's properties, the curve layouts, the host refusals, and the refusal of every device entry
without a device."""
import ctypes as C
import json

import numpy as np
import pytest

import rank_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import link_classification as LC
from gem_amd.evaluation import ranking as RK
from gem_amd.graph import EdgeListGraph

ULP = 2.0 ** -52


@pytest.fixture(scope='module')
def fixture():
    return json.load(open(golden_path('link_auc_ref.json'))), np.load(golden_path('link_auc_ref.npz'))


@pytest.fixture(scope='module')
def sets():
    out = R.metric_sets()
    out['curve'] = R.curve_set()
    return out


@pytest.fixture(scope='module')
def exact(sets):
    return {name: R.exact_scores(s, y) for name, (s, y) in sets.items()}


def test_exact_restatement_against_sklearn(sets, exact, fixture):
    from sklearn.metrics import average_precision_score, roc_auc_score
    tol = 4 * fixture[0]['sklearn_metrics_vs_exact']
    assert 0 < tol < 1e-15
    for name, (s, y) in sets.items():
        ex = exact[name]
        assert abs(roc_auc_score(y, s) - float(ex['auc'])) <= tol, name
        assert abs(average_precision_score(y, s) - float(ex['ap'])) <= tol, name
        assert ex['P'] + ex['N'] == len(s) and ex['T'] == len(np.unique(s))
    assert exact['separated_up']['auc'] == 1 and exact['separated_down']['auc'] == 0
    assert float(exact['all_tied']['auc']) == 0.5 and exact['all_tied']['ap'] * (exact['all_tied']['P'] + exact['all_tied']['N']) == exact['all_tied']['P']
    assert exact['one_positive_first']['auc'] == 1 and exact['one_positive_last']['auc'] == 0


def test_argsort_restatement_orders_zeros_infinities_and_ties():
    s = np.array([0.0, -0.0, np.inf, 1.0, -np.inf, 1.0, -0.0, 0.0, np.inf])
    assert R.argsort_ref(s).tolist() == [2, 8, 3, 5, 0, 1, 6, 7, 4]


def test_operator_restatements_round_every_step_to_float32():
    rng = np.random.RandomState(0)
    A = rng.standard_normal((50, 7)).astype(np.float32); B = rng.standard_normal((50, 7)).astype(np.float32)
    for op in R.OPS:
        assert R.op_ref(op, A, B).dtype == np.float32
    t = (A - B)
    assert np.array_equal(R.op_ref('l2', A, B), t * t) and np.array_equal(R.op_ref('l1', A, B), np.abs(t))
    wide = (A.astype(np.float64) - B.astype(np.float64)) ** 2
    assert not np.array_equal(R.op_ref('l2', A, B).astype(np.float64), wide)           # the rounded difference is what is squared
    assert np.array_equal(R.op_ref('average', A, B), ((A.astype(np.float64) + B) .astype(np.float32) * np.float32(0.5)))


def test_host_metrics_from_groups_against_the_exact_rationals(sets, exact):
    for name, ex in exact.items():
        got = RK.binary_scores_from_groups(ex['tp'], ex['fp'])
        assert (got['n_pos'], got['n_neg'], got['n_thresholds'], got['u2']) == (ex['P'], ex['N'], ex['T'], ex['U2']), name
        assert abs(got['auc'] - float(ex['auc'])) <= ULP * float(ex['auc']), name
        assert abs(got['ap'] - float(ex['ap'])) <= 4 * ex['T'] * 2.0 ** -53 * float(ex['ap']), name
        assert got['prevalence'] == ex['P'] / float(ex['P'] + ex['N'])
    got = RK.binary_scores_from_groups([3, 3], [0, 5])
    assert got['auc'] == 1.0 and got['ap'] == 1.0
    got = RK.binary_scores_from_groups([0, 3], [5, 5])
    assert got['auc'] == 0.0 and got['ap'] == 3 / 8.0


def test_host_metrics_refuse_a_bad_group_table():
    for tp, fp, words in (([], [], 'T = 0'), ([1, 1], [1, 1], 'group 1 = (1, 1)'), ([2, 1], [0, 3], 'group 1 = (1, 3)'), ([0, 0], [1, 2], 'no positive'),
                          ([1, 2], [0, 0], 'no negative'), ([1, 2 ** 31], [1, 2], 'group 1')):
        with pytest.raises(_hip.GemHipError, match='error -1') as e:
            RK.binary_scores_from_groups(tp, fp)
        assert words in str(e.value), (tp, fp, str(e.value))


def test_curve_layouts_against_sklearn_on_a_tied_set(exact, fixture):
    from sklearn.metrics import precision_recall_curve, roc_curve
    s, y = R.curve_set()
    ex = exact['curve']
    assert ex['T'] < len(s) // 4                                       # heavy ties
    fpr, tpr, thr = RK.roc_from_groups(ex['thr'], ex['tp'], ex['fp'])
    prec, rec, pthr = RK.pr_from_groups(ex['thr'], ex['tp'], ex['fp'])
    tol = 4 * fixture[0]['curve']['sklearn_vs_exact']
    want = roc_curve(y, s, drop_intermediate=False) + precision_recall_curve(y, s)
    for got, ref in zip((fpr, tpr, thr, prec, rec, pthr), want):
        assert got.shape == ref.shape
        assert np.all(np.abs(got[np.isfinite(ref)] - ref[np.isfinite(ref)]) <= tol)
    assert thr[0] == np.inf and (fpr[0], tpr[0]) == (0.0, 0.0) and (prec[-1], rec[-1]) == (1.0, 0.0)
    for key, got in (('roc_fpr', fpr), ('roc_tpr', tpr), ('pr_precision', prec), ('pr_recall', rec)):
        assert np.all(np.abs(got - fixture[1][key]) <= tol)


def ring(n, extra=()):
    u = np.arange(n); v = (u + 1) % n
    st = np.concatenate([u, v, [a for a, b in extra], [b for a, b in extra]]); ed = np.concatenate([v, u, [b for a, b in extra], [a for a, b in extra]])
    return EdgeListGraph(n, st, ed)


def test_sample_non_edges_properties():
    g = ring(200, extra=[(0, 50), (3, 3)])
    arcs = set(zip(g.src.tolist(), g.dst.tolist()))
    st, ed = LC.sample_non_edges(g, 3000, seed=4)
    assert st.dtype == np.int32 and len(st) == 3000 and np.all(st < ed) and st.min() >= 0 and ed.max() < 200
    got = list(zip(st.tolist(), ed.tolist()))
    assert len(set(got)) == 3000
    assert not any((a, b) in arcs or (b, a) in arcs for a, b in got)
    st2, ed2 = LC.sample_non_edges(g, 3000, seed=4)
    assert np.array_equal(st, st2) and np.array_equal(ed, ed2)
    st3, _ = LC.sample_non_edges(g, 3000, seed=5)
    assert not np.array_equal(st, st3)
    ex_st, ex_ed = LC.sample_non_edges(g, 2500, seed=6, exclude=(ed, st))            # the excluded pairs given in the other orientation
    assert not set(zip(ex_st.tolist(), ex_ed.tolist())) & set(got)
    assert len(LC.sample_non_edges(g, 0, seed=1)[0]) == 0


def test_sample_non_edges_directed_keeps_the_orientation():
    g = EdgeListGraph(30, np.arange(29), np.arange(1, 30))             # a directed path
    st, ed = LC.sample_non_edges(g, 400, seed=2, is_undirected=False)
    got = set(zip(st.tolist(), ed.tolist()))
    assert len(got) == 400 and all(a != b and b != a + 1 for a, b in got)
    assert any(a == b + 1 for a, b in got)                             # the reverse of an arc is a legal non-edge
    assert np.any(st > ed)


def test_sample_non_edges_refuses_a_dense_graph():
    n = 12
    u, v = np.triu_indices(n, 1)
    full = EdgeListGraph(n, np.concatenate([u, v]), np.concatenate([v, u]))
    with pytest.raises(ValueError, match='0 non-edges exist'):
        LC.sample_non_edges(full, 1, seed=0)
    almost = EdgeListGraph(n, np.concatenate([u[6:], v[6:]]), np.concatenate([v[6:], u[6:]]))         # six non-edges: three may be sampled
    assert len(LC.sample_non_edges(almost, 3, seed=0)[0]) == 3
    with pytest.raises(ValueError, match='4 pairs asked for, 6 non-edges exist'):
        LC.sample_non_edges(almost, 4, seed=0)
    with pytest.raises(ValueError, match='3 non-edges exist'):
        LC.sample_non_edges(almost, 2, seed=0, exclude=(u[:3], v[:3]))


def test_link_pairs_of_the_fixture_split(fixture):
    train, test, pairs = R.fixture_pairs()
    meta = fixture[0]
    assert [pairs[k] for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg')] == [meta[k] for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg')]
    assert pairs['n_train_pos'] + pairs['n_test_pos'] == 21045 and pairs['n_train_neg'] == pairs['n_train_pos'] and pairs['n_test_neg'] == pairs['n_test_pos']
    n = pairs['n']

    def keys(part, lab):
        st, ed, y = pairs[part]
        assert np.all(st < ed)
        return set((st[y == lab].astype(np.int64) * n + ed[y == lab]).tolist())
    assert keys('train', 1) == arcs_of(train, n) and keys('test', 1) == arcs_of(test, n)
    assert not keys('train', 0) & keys('test', 0)
    assert not (keys('train', 0) | keys('test', 0)) & (arcs_of(train, n) | arcs_of(test, n))
    sub = LC.link_pairs(train, test, seed=0, max_train_pairs=500, neg_ratio=2.0)
    assert (sub['n_train_pos'], sub['n_train_neg']) == (500, 1000)
    assert set(zip(sub['train'][0][:500].tolist(), sub['train'][1][:500].tolist())) <= set(zip(pairs['train'][0].tolist(), pairs['train'][1].tolist()))


def arcs_of(g, n):
    return set((np.minimum(g.src, g.dst).astype(np.int64) * n + np.maximum(g.src, g.dst)).tolist())


# ------------------------------------------------------------------ refusals decided on the host, before any device call
def rank_call(fn, s, y=None):
    L = _hip.lib()
    s = np.ascontiguousarray(s, dtype=np.float64)
    m = len(s)
    perm = np.zeros(max(m, 1), np.int32); out = (C.c_double * 4)(); cnt = (C.c_int64 * 4)(); T = C.c_int64(-5)
    if fn == 'argsort':
        return L.gemhip_rank_argsort(m, _hip.ptr(s, C.c_double), _hip.ptr(perm, C.c_int32))
    y = np.ascontiguousarray(y, dtype=np.uint8)
    if fn == 'binary':
        return L.gemhip_rank_binary(m, _hip.ptr(s, C.c_double), _hip.ptr(y, C.c_uint8), out, cnt)
    thr = np.zeros(max(m, 1)); tp = np.zeros(max(m, 1), np.int64); fp = np.zeros(max(m, 1), np.int64)
    return L.gemhip_rank_curve(m, _hip.ptr(s, C.c_double), _hip.ptr(y, C.c_uint8), m, _hip.ptr(thr, C.c_double), _hip.ptr(tp, C.c_int64), _hip.ptr(fp, C.c_int64),
                               C.byref(T))


def test_rank_host_refusals_name_the_position():
    L = _hip.lib()
    s = np.array([0.5, 1.0, np.nan, 2.0, np.nan])
    for fn, who in (('argsort', b'rank_argsort'), ('binary', b'rank_binary'), ('curve', b'rank_curve')):
        assert rank_call(fn, s, [0, 1, 0, 1, 0]) == _hip.E_INVALID
        assert L.gemhip_last_error() == who + b': score[2] is NaN'
        assert rank_call(fn, np.zeros(0), np.zeros(0)) == _hip.E_INVALID
        assert L.gemhip_last_error() == who + b': m = 0 (need m >= 1)'
    ok = np.array([0.5, 1.0, np.inf, -np.inf])
    for fn, who in (('binary', b'rank_binary'), ('curve', b'rank_curve')):
        assert rank_call(fn, ok, [0, 1, 2, 1]) == _hip.E_INVALID
        assert L.gemhip_last_error() == who + b': label[2] = 2 is neither 0 nor 1'
        assert rank_call(fn, ok, [0, 0, 0, 0]) == _hip.E_INVALID
        assert L.gemhip_last_error() == who + b': only one class present: no positive label among 4'
        assert rank_call(fn, ok, [1, 1, 1, 1]) == _hip.E_INVALID
        assert L.gemhip_last_error() == who + b': only one class present: no negative label among 4'
    with pytest.raises(ValueError, match=r'label\[1\] = 3'):
        RK.binary_ranking_scores([0.1, 0.2], [0, 3])


def edgeclf_create(X, d=None):
    L = _hip.lib()
    X = np.ascontiguousarray(X, dtype=np.float32)
    h = C.c_void_p()
    rc = L.gemhip_edgeclf_create(X.shape[0], X.shape[1] if d is None else d, X.shape[1], _hip.ptr(X, C.c_float), C.byref(h))
    return rc, h


def test_edgeclf_create_refusals():
    L = _hip.lib()
    rc, h = edgeclf_create(np.zeros((3, 256)))
    assert rc == _hip.E_UNSUPPORTED and not h.value and b'd = 256: at most 255' in L.gemhip_last_error()
    X = np.ones((4, 3)); X[2, 1] = np.inf
    rc, h = edgeclf_create(X)
    assert rc == _hip.E_INVALID and not h.value and L.gemhip_last_error() == b'edgeclf_create: X[2][1] is not finite'
    X[2, 1] = -2e18
    rc, h = edgeclf_create(X)
    assert rc == _hip.E_INVALID and b'|X[2][1]|' in L.gemhip_last_error()
    X[2, 1] = np.nan
    rc, h = edgeclf_create(X, d=1)                                      # NaN in the padding is never looked at: the next failure is the device's
    if _hip.device_count() == 0:
        assert rc == _hip.E_HIP and not h.value
    else:
        assert rc == 0
        L.gemhip_edgeclf_destroy(h)
    assert edgeclf_create(np.zeros((3, 2)), d=3)[0] == _hip.E_INVALID
    with pytest.raises(ValueError, match="operator 'cosine'"):
        LC._op_id('cosine')


def test_every_device_entry_raises_without_a_device():
    if _hip.device_count() > 0:
        pytest.skip('GPU present')
    s = np.linspace(0, 1, 10); y = np.arange(10) % 2
    for call in (lambda: RK.argsort_desc(s), lambda: RK.binary_ranking_scores(s, y), lambda: RK.roc_curve(s, y), lambda: RK.precision_recall_curve(s, y),
                 lambda: LC.EdgeClassifier(np.zeros((4, 2), np.float32)),
                 lambda: LC.evaluate_link_classification(ring(8), ring(8), np.zeros((8, 2), np.float32))):
        with pytest.raises(_hip.GemHipError):
            call()
    assert RK.sort_info()['keys_per_workgroup'] >= 256                 # a constant: no device needed
