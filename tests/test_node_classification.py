"""CPU tier of node classification (tests/README_nc.md): the numpy-only helpers, the restatements against sklearn, the host Newton step,
the fixtures, and the refusal of every device entry without a device."""
import ctypes as C
import json

import numpy as np
import pytest

import nc_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import node_classification as NC
from gem_amd.graph import sbm_block_labels


def test_label_csr_takes_three_forms():
    import scipy.sparse as sp
    Y = np.array([[0, 1, 1], [0, 0, 0], [1, 0, 0], [0, 0, 1]], np.uint8)
    want = (3, [0, 2, 2, 3, 4], [1, 2, 0, 2])
    for form in (Y, Y.astype(np.float64), sp.csr_matrix(Y), sp.coo_matrix(Y)):
        K, rp, cls = NC.label_csr(form, 4)
        assert (K, rp.tolist(), cls.tolist()) == want and rp.dtype == np.int64 and cls.dtype == np.int32
    K, rp, cls = NC.label_csr(np.array([2, 0, 1, 2], np.int16), 4)
    assert (K, rp.tolist(), cls.tolist()) == (3, [0, 1, 2, 3, 4], [2, 0, 1, 2])
    explicit_zero = sp.csr_matrix((np.array([1.0, 0.0]), np.array([1, 2]), np.array([0, 2, 2])), shape=(2, 3))
    assert NC.label_csr(explicit_zero, 2)[2].tolist() == [1]


def test_label_csr_refusals():
    with pytest.raises(ValueError, match=r'Y\[1\]\[0\] is neither 0 nor 1'):
        NC.label_csr(np.array([[0, 1], [2, 0]]), 2)
    with pytest.raises(ValueError, match='negative label -1 at node 1'):
        NC.label_csr(np.array([0, -1]), 2)
    with pytest.raises(ValueError, match='integers'):
        NC.label_csr(np.array([0.0, 1.0]), 2)
    with pytest.raises(ValueError, match='expected 3'):
        NC.label_csr(np.array([0, 1]), 3)
    with pytest.raises(ValueError):
        NC.label_csr(np.zeros((2, 2, 2)), 2)


def test_split_nodes_counts():
    for n, ratio in ((10, 0.25), (1024, 0.3), (1024, 0.1), (7, 0.5), (100, 0.9)):
        tr, te = NC.split_nodes(n, ratio, 3)
        assert len(te) == int(np.ceil(ratio * n)) and len(tr) == n - len(te)
        assert sorted(np.concatenate([tr, te]).tolist()) == list(range(n))
        assert np.array_equal(np.concatenate([te, tr]), np.random.RandomState(3).permutation(n))
    assert np.array_equal(NC.split_nodes(1024, R.TEST_RATIO, R.SPLIT_SEED)[0], R.split(1024)[0])
    for bad in (0.0, 1.0, -0.1, 1e-9 - 1):
        with pytest.raises(ValueError):
            NC.split_nodes(10, bad, 0)
    with pytest.raises(ValueError):
        NC.split_nodes(2, 0.9, 0)


def test_sbm_block_labels():
    assert sbm_block_labels(6, 3).tolist() == [0, 0, 1, 1, 2, 2]
    assert sbm_block_labels(7, 3).tolist() == [0, 0, 1, 1, 2, 2, 2]
    assert np.array_equal(sbm_block_labels(1000, 10), np.arange(1000) // 100)


def check_metrics(pred, Y):
    from sklearn.metrics import accuracy_score, f1_score
    tp, fp, fn, exact = R.counts_ref(pred, Y)
    micro, macro = NC.f1_from_counts(tp, fp, fn)
    assert micro == pytest.approx(f1_score(Y, pred, average='micro', zero_division=0), abs=1e-15)
    assert macro == pytest.approx(f1_score(Y, pred, average='macro', zero_division=0), abs=1e-15)
    assert exact / len(Y) == pytest.approx(accuracy_score(Y, pred), abs=1e-15)
    return micro, macro, exact / len(Y)


def test_metrics_and_topk_against_sklearn_on_the_fixture():
    ref = json.load(open(golden_path('nc_ref.json')))
    W = np.load(golden_path('nc_ref.npz'))
    sets = R.data_sets()
    for name in ('std', 'x100'):
        ds = sets[name]
        test = R.split(len(ds['X']))[1]
        Y = ds['Y'][test]
        pred = R.topk_ref(R.scores_ref(ds['X'][test], W['W_' + name]), Y.sum(1))
        micro, macro, acc = check_metrics(pred, Y)
        want = ref['sets'][name]
        assert (micro, macro, acc) == (want['micro'], want['macro'], want['accuracy'])
        tp, fp, fn, exact = R.counts_ref(pred, Y)
        assert (tp.tolist(), fp.tolist(), fn.tolist(), exact) == (want['tp'], want['fp'], want['fn'], want['exact'])


def test_metrics_with_an_empty_class_and_a_row_without_labels():
    Y = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]], np.uint8)        # classes 2, 3: no true label; row 2: k = 0
    scores = np.array([[0.1, 0.9, 0.2, -1.0], [0.0, 0.5, 0.5, -1.0], [3.0, 2.0, 1.0, 0.0], [1.0, 1.0, 1.0, -1.0]])
    pred = R.topk_ref(scores, Y.sum(1))
    assert pred.tolist() == [[0, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], [1, 1, 0, 0]]            # row 1: the tie 0.5 / 0.5 goes to class 1
    micro, macro, acc = check_metrics(pred, Y)
    tp, fp, fn, _ = R.counts_ref(pred, Y)
    assert (tp + fp + fn)[3] == 0 and (tp + fp + fn)[2] == 0
    assert macro == pytest.approx((2 * 1 / 3 + 2 * 2 / 5) / 4) and acc == 0.75
    assert NC.f1_from_counts([0, 0], [0, 0], [0, 0]) == (0.0, 0.0)


def host_step(H, g):
    return NC.newton_step_host(H, g)


def test_newton_step_host_against_numpy():
    rng = np.random.RandomState(0)
    for d1 in (1, 2, 33, 129):
        A = rng.standard_normal((3 * d1 + 2, d1))
        H = A.T @ A / len(A) + np.eye(d1)
        g = rng.standard_normal(d1)
        delta, dec, shift = host_step(H, g)
        want = np.linalg.solve(H, -g)
        assert shift == 0.0
        assert np.abs(delta - want).max() <= 1e-13 * np.linalg.cond(H) * np.abs(want).max()
        assert dec == pytest.approx(-(g @ want), rel=1e-12)
        lower_garbage = np.triu(H) + np.tril(rng.standard_normal((d1, d1)), -1)              # only the upper triangle is read
        assert np.array_equal(host_step(lower_garbage, g)[0], delta)


def test_newton_step_host_near_singular():
    rng = np.random.RandomState(1)
    d1 = 20
    Q, _ = np.linalg.qr(rng.standard_normal((d1, d1)))
    H = (Q * np.logspace(0, -10, d1)) @ Q.T
    H = (H + H.T) / 2
    g = rng.standard_normal(d1)
    delta, dec, shift = host_step(H, g)
    assert shift == 0.0
    want = np.linalg.solve(H, -g)
    cond = np.linalg.cond(H)
    assert np.abs(delta - want).max() <= 64 * np.finfo(float).eps * cond * np.abs(want).max()
    assert np.abs(H @ delta + g).max() <= 64 * np.finfo(float).eps * (np.abs(H).sum(1).max() * np.abs(delta).max() + np.abs(g).max()) * d1
    assert dec > 0


def test_newton_step_host_levenberg_on_an_indefinite_matrix():
    rng = np.random.RandomState(2)
    d1 = 12
    Q, _ = np.linalg.qr(rng.standard_normal((d1, d1)))
    lam = np.linspace(1.0, 5.0, d1); lam[0] = -0.5
    H = (Q * lam) @ Q.T
    H = (H + H.T) / 2
    g = rng.standard_normal(d1)
    delta, dec, shift = host_step(H, g)
    base = 1e-10 * max(1.0, np.abs(np.diag(H)).max())       # the ladder base * 10^k: the first rung past -lambda_min = 0.5
    k = int(round(np.log10(shift / base)))
    assert shift == pytest.approx(base * 10.0 ** k, rel=1e-12) and shift > 0.5 and shift / 10 <= 0.5
    want = np.linalg.solve(H + shift * np.eye(d1), -g)
    assert np.abs(delta - want).max() <= 1e-12 * np.linalg.cond(H + shift * np.eye(d1)) * np.abs(want).max()
    assert dec > 0                                         # a descent direction
    L = _hip.lib()
    bad = H.copy(); bad[0, 1] = np.nan
    out = np.zeros(d1); dec_c = C.c_double()
    assert L.gemhip_nc_newton_step_host(d1, _hip.ptr(bad, C.c_double), _hip.ptr(g, C.c_double), _hip.ptr(out, C.c_double), C.byref(dec_c), None) == _hip.E_NOTCONVERGED
    assert L.gemhip_nc_newton_step_host(0, _hip.ptr(H, C.c_double), _hip.ptr(g, C.c_double), _hip.ptr(out, C.c_double), C.byref(dec_c), None) == _hip.E_INVALID


def test_restated_fp64_fit_against_the_fixture():
    W = np.load(golden_path('nc_ref.npz'))
    sets = R.data_sets()
    for name in ('std', 'raw', 'normal', 'normal_C1e4', 'warm'):
        ds = sets[name]
        train = R.train_rows(name, len(ds['X']))
        got, info = R.fit_all(ds['X'][train], ds['Y'][train], ds['C'], ds['W0'], np.float64, dec_tol=1e-12)
        want = W['W_' + name]
        assert all(i['converged'] for i in info)
        assert (np.abs(got - want).max(1) / np.abs(want).max(1)).max() <= 1e-12, name
        if name in R.LINE_SEARCH_SETS:
            assert sum(i['backtracks'] for i in info) >= 1


def test_fixtures_load_with_the_stated_shapes():
    W = np.load(golden_path('nc_ref.npz'))
    ref = json.load(open(golden_path('nc_ref.json')))
    sets = R.data_sets()
    assert sorted(W.files) == sorted('W_' + k for k in sets) and sorted(ref['sets']) == sorted(sets)
    for name, ds in sets.items():
        assert W['W_' + name].shape == (ds['Y'].shape[1], ds['X'].shape[1] + 1) and W['W_' + name].dtype == np.float64
        assert ds['X'].dtype == np.float32 and np.isfinite(W['W_' + name]).all()
    assert sets['std']['Y'].shape == (1024, 8) and sets['warm']['X'].shape == (1061, 33) and sets['normal']['X'].shape == (300, 128)
    for name in ('std', 'x100'):
        e = ref['sets'][name]
        assert e['min_probability_gap'] >= 4 * e['float32_probability_deviation'] and e['default_settings_identical'] is True


def test_device_entries_raise_without_a_device():
    if _hip.device_count() > 0:
        pytest.skip('GPU present')
    X = np.zeros((4, 2), np.float32)
    with pytest.raises(_hip.GemHipError):
        NC.NodeClassifier(X)
    with pytest.raises(_hip.GemHipError):
        NC.evaluateNodeClassification(X, np.array([0, 1, 0, 1]), 0.5)
    with pytest.raises(_hip.GemHipError):
        NC.expNC(X, np.array([0, 1, 0, 1]), [0.5], 1)
    from gem.evaluation import evaluate_node_classification as alias
    assert alias.evaluateNodeClassification is NC.evaluateNodeClassification and alias.expNC is NC.expNC


def test_create_refuses_on_the_host_before_any_device_call():
    """Validation only: these return before the first HIP call, so they run without a GPU."""
    L = _hip.lib()
    h = C.c_void_p()
    X = np.ones((3, 4), np.float32); X[2, 1] = np.nan

    def create(n, d, ld, A):
        return L.gemhip_nc_create(n, d, ld, _hip.ptr(A, C.c_float), C.byref(h))
    assert create(3, 4, 4, X) == _hip.E_INVALID and L.gemhip_last_error() == b'nc_create: X[2][1] is not finite'
    X[2, 1] = np.inf
    assert create(3, 4, 4, X) == _hip.E_INVALID and L.gemhip_last_error() == b'nc_create: X[2][1] is not finite'
    assert create(3, 0, 4, X) == _hip.E_INVALID and create(3, 4, 3, X) == _hip.E_INVALID and create(0, 4, 4, X) == _hip.E_INVALID
    assert create(3, 256, 256, X) == _hip.E_UNSUPPORTED and b'd = 256: at most 255' in L.gemhip_last_error()
    assert create(2 ** 31, 4, 4, X) == _hip.E_UNSUPPORTED and b'below 2^31' in L.gemhip_last_error()
    assert not h.value
