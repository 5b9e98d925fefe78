"""GPU tier of node classification (tests/README_nc.md): the pass kernel stage by stage, the fit against the exact minimiser, degenerate
classes, the top-k ranker and its counts, the public entry points end to end, determinism and the refusals."""
import json
import warnings

import numpy as np
import pytest

import nc_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import node_classification as NC

pytestmark = pytest.mark.gpu

SLAB = 64                        # rows per LDS sub-slab (gemhip_nc_info[7]); 512 rows are one workgroup's share: 1061 rows make three, the last of 37
CLASS_BLOCK = 4                  # classes per kernel block (gemhip_nc_info[6])
CHAIN_FACTOR = 1.0               # the guide's 0.75-1.5e-7 holds for chains up to 1024 terms, which is the longest the kernel makes
B_MFMA = 4 * 1.5e-7 * CHAIN_FACTOR


@pytest.fixture(scope='module')
def sets():
    return R.data_sets()


@pytest.fixture(scope='module')
def golden():
    return np.load(golden_path('nc_ref.npz')), json.load(open(golden_path('nc_ref.json')))


def padded(X, extra=3):
    """X in a wider array whose padding columns are NaN: the device must never read them."""
    out = np.full((X.shape[0], X.shape[1] + extra), np.nan, np.float32)
    out[:, :X.shape[1]] = X
    return out


def test_kernel_constants_are_the_ones_the_shapes_below_were_chosen_for():
    with NC.NodeClassifier(np.zeros((2, 1), np.float32)) as nc:
        st = nc.stats()
    assert (st['slab_rows'], st['class_block']) == (SLAB, CLASS_BLOCK)


def check_pass(nc, X, Y, train, W, Creg, tag):
    F, g, H = nc.pass_(train, W, C=Creg)
    Xa = R.augment(X[train], np.float64)
    ax = np.abs(Xa)
    for c in range(Y.shape[1]):
        Fr, gr, Hr = R.pass_ref(Xa, Y[train, c], W[c], Creg)
        z = Xa @ W[c]
        p, q, _ = R.sigma_parts(z)
        r = np.where(Y[train, c] > 0, q, p)
        bound_g = B_MFMA * Creg * (ax.T @ r) + 4 * np.finfo(float).eps * np.abs(W[c])
        bound_H = B_MFMA * Creg * ((ax * (p * q)[:, None]).T @ ax) + 4 * np.finfo(float).eps * np.abs(Hr)          # ... and the fp64 assembly
        eg, eH, eF = np.abs(g[c] - gr), np.abs(H[c] - Hr), abs(F[c] - Fr) / abs(Fr)
        print('%s class %d: g err/bound %.2e  H err/bound %.2e  F rel %.2e' % (tag, c, (eg / bound_g).max(), (eH / np.maximum(bound_H, 1e-300)).max(), eF))
        assert np.all(eg <= bound_g), tag
        assert np.all(eH <= bound_H), tag
        assert eF <= 1e-6, tag
        assert np.array_equal(H[c], H[c].T)


def pass_case(d, n_trains, Ks, seed):
    rng = np.random.RandomState(seed)
    n = 1200
    X = rng.standard_normal((n, d)).astype(np.float32)
    with NC.NodeClassifier(padded(X), d=d) as nc:
        for K in Ks:
            Y = R.random_labels(n, K, seed + K)
            nc.set_labels(Y)
            for n_train in n_trains:
                train = rng.permutation(n)[:n_train].astype(np.int32)              # shuffled
                if n_train > 1:
                    train[-1] = train[0]                                            # a repeated row counts twice
                for W in (np.zeros((K, d + 1)), rng.standard_normal((K, d + 1))):
                    check_pass(nc, X, Y, train, W, 1.0, 'd=%d n_train=%d K=%d W%s' % (d, n_train, K, '=0' if not W.any() else '~N(0,1)'))


@pytest.mark.parametrize('d', [1, 2, 32, 33, 128, 131])
def test_pass_every_width(d):
    """d + 1 below, at and above the 32-wide tile, one to five tiles; several workgroups with a ragged last one; a class block and one more."""
    pass_case(d, (1061,), (CLASS_BLOCK + 1,), 100 + d)


def test_pass_every_row_count_and_class_count():
    pass_case(33, (1, SLAB - 1, SLAB, SLAB + 1, 1061), (3,), 7)
    pass_case(32, (SLAB + 1,), (1, CLASS_BLOCK + 1), 8)


def test_pass_scales_with_C():
    rng = np.random.RandomState(3)
    X = rng.standard_normal((200, 5)).astype(np.float32)
    Y = R.random_labels(200, 2, 4)
    with NC.NodeClassifier(X) as nc:
        nc.set_labels(Y)
        check_pass(nc, X, Y, np.arange(200, dtype=np.int32), rng.standard_normal((2, 6)), 1e4, 'C=1e4')


@pytest.fixture(scope='module')
def fits(sets, golden):
    """One device fit per coefficient set, shared by the tests below."""
    out = {}
    for name in ('std', 'raw', 'normal', 'normal_C1e4', 'warm'):
        ds = sets[name]
        train = R.train_rows(name, len(ds['X']))
        with NC.NodeClassifier(ds['X']) as nc:
            nc.set_labels(ds['Y'])
            out[name] = nc.fit(train, C=ds['C'], W0=ds['W0']) + (train,)
    return out


@pytest.mark.parametrize('name', ['std', 'raw', 'normal', 'normal_C1e4', 'warm'])
def test_fit_against_the_exact_minimiser(name, sets, golden, fits):
    ds, Wstar = sets[name], golden[0]['W_' + name]
    coef, intercept, info, train = fits[name]
    W = np.hstack([coef, intercept[:, None]])
    scale = np.abs(Wstar).max(1)
    W32 = R.fit_all(ds['X'][train], ds['Y'][train], ds['C'], ds['W0'], np.float32)[0]
    dev32 = (np.abs(W32 - Wstar).max(1) / scale).max()
    Xa = R.augment(ds['X'][train], np.float64)
    derived = 0.0
    for c in range(len(Wstar)):                           # |H^-1|_inf * delta g, delta g the f32 matrix units' error on the gradient's own terms
        _, _, H = R.pass_ref(Xa, ds['Y'][train, c], Wstar[c], ds['C'])
        p, q, _ = R.sigma_parts(Xa @ Wstar[c])
        dg = B_MFMA * ds['C'] * (np.abs(Xa).T @ np.where(ds['Y'][train, c] > 0, q, p)).max()
        derived = max(derived, np.abs(np.linalg.inv(H)).sum(1).max() * dg / scale[c])
    dev = (np.abs(W - Wstar).max(1) / scale).max()
    print('%s: device %.3e   4 x float32 restatement %.3e   derived %.3e   iterations %s backtracks %s' %
          (name, dev, 4 * dev32, derived, info['iterations'].tolist(), info['backtracks'].tolist()))
    assert dev <= max(4 * dev32, derived)
    assert info['converged'].all() and not info['degenerate'].any()
    assert (info['iterations'] >= 1).all() and info['passes'] == info['iterations'].max()
    if name in R.LINE_SEARCH_SETS:
        assert info['backtracks'].sum() > 0 and info['loss_evaluations'] > 0


def test_unconverged_fit_warns_and_returns_its_iterate(sets):
    ds = sets['std']
    train = R.train_rows('std', 1024)
    with NC.NodeClassifier(ds['X']) as nc:
        nc.set_labels(ds['Y'])
        with pytest.warns(RuntimeWarning, match='not converged'):
            coef, _, info = nc.fit(train, max_iter=2)
    assert not info['converged'].any() and (info['iterations'] == 2).all() and np.isfinite(coef).all()


def test_degenerate_classes_leave_the_others_untouched(sets, fits):
    ds = sets['std']
    train = R.train_rows('std', 1024)
    Y = ds['Y']
    absent = np.zeros(len(Y), np.uint8); absent[np.setdiff1d(np.arange(len(Y)), train)[:5]] = 1           # positives on test rows only
    everywhere = np.zeros(len(Y), np.uint8); everywhere[train] = 1
    Y10 = np.column_stack([Y[:, :1], absent, Y[:, 1:5], everywhere, Y[:, 5:]])
    keep = [0, 2, 3, 4, 5, 7, 8, 9]
    with NC.NodeClassifier(ds['X']) as nc:
        nc.set_labels(Y10)
        coef, intercept, info = nc.fit(train, W0=np.ones((10, 33)))
        coef0, intercept0, info0 = nc.fit(train)
    assert info['degenerate'].tolist() == [0, -1, 0, 0, 0, 0, 1, 0, 0, 0] and info['converged'].all()
    for c, b in ((1, -np.inf), (6, np.inf)):
        assert not coef0[c].any() and intercept0[c] == b and info0['iterations'][c] == 0
        assert not coef[c].any() and intercept[c] == b                                                      # whatever the start was
    assert np.array_equal(coef0[keep], fits['std'][0]) and np.array_equal(intercept0[keep], fits['std'][1])
    assert np.array_equal(info0['iterations'][keep], fits['std'][2]['iterations'])


def check_topk(nc, X, Y, W, rows, k=None):
    nc.set_weights(W)
    scores = nc.decision_function(rows)
    want_scores = R.scores_ref(X[rows], W)
    finite = np.isfinite(want_scores)
    assert np.array_equal(scores[~finite], want_scores[~finite])
    assert np.abs(scores[finite] - want_scores[finite]).max() <= 1e-13 * max(1.0, np.abs(want_scores[finite]).max())
    pred, tp, fp, fn, exact = nc.predict_topk(rows, k)
    kk = Y[rows].sum(1) if k is None else k
    want = R.topk_ref(scores, kk)
    assert np.array_equal(pred, want)
    wtp, wfp, wfn, wexact = R.counts_ref(pred, Y[rows])
    assert (tp.tolist(), fp.tolist(), fn.tolist(), exact) == (wtp.tolist(), wfp.tolist(), wfn.tolist(), wexact)
    none, tp2, fp2, fn2, exact2 = nc.predict_topk(rows, k, want_pred=False)
    assert none is None and (tp2.tolist(), fp2.tolist(), fn2.tolist(), exact2) == (wtp.tolist(), wfp.tolist(), wfn.tolist(), wexact)
    return tp, fp, fn, exact


def test_topk_and_counts_on_the_fixture(sets, golden):
    for name in ('std', 'x100'):
        ds, want = sets[name], golden[1]['sets'][name]
        test = R.split(1024)[1]
        with NC.NodeClassifier(ds['X']) as nc:
            nc.set_labels(ds['Y'])
            tp, fp, fn, exact = check_topk(nc, ds['X'], ds['Y'], golden[0]['W_' + name], test)
        assert (tp.tolist(), fp.tolist(), fn.tolist(), exact) == (want['tp'], want['fp'], want['fn'], want['exact'])


def test_topk_ties_infinities_and_k_extremes():
    """Small integers in X and W: every logit is exact in fp64 whatever the summation order, so equal logits are equal on the device too."""
    rng = np.random.RandomState(11)
    n, d, K = 70, 3, 6
    X = rng.randint(-2, 3, (n, d)).astype(np.float32)
    W = rng.randint(-1, 2, (K, d + 1)).astype(np.float64)
    W[1] = W[0]                                   # classes 0 and 1 tie on every row
    W[4, :d] = 0; W[4, d] = -np.inf               # constant predictors
    W[5, :d] = 0; W[5, d] = np.inf
    Y = R.random_labels(n, K, 12)
    Y[0] = 0                                      # a row without labels: k = 0 by default
    Y[1] = 1                                      # a row with every label: k = K
    rows = rng.permutation(n).astype(np.int32)
    with NC.NodeClassifier(X) as nc:
        nc.set_labels(Y)
        check_topk(nc, X, Y, W, rows)
        pred = nc.predict_topk(np.array([0, 1], np.int32))[0]
        assert not pred[0].any() and pred[1].all()
        k = rng.randint(0, K + 1, n).astype(np.int32); k[:3] = (0, K, 1)
        check_topk(nc, X, Y, W, rows, k)
        pred = nc.predict_topk(rows, np.ones(n, np.int32))[0]
        assert pred[:, 5].all() and pred.sum() == n            # +inf wins alone
        pred = nc.predict_topk(rows, np.full(n, 3, np.int32))[0]
        assert np.all(pred[:, 0] >= pred[:, 1]) and not pred[:, 4].any()          # the lower id first; -inf never among 3 of 6


def test_end_to_end_equals_the_fixture_metrics(sets, golden):
    from gem.evaluation.evaluate_node_classification import evaluateNodeClassification
    for name in ('std', 'x100'):
        ds, want = sets[name], golden[1]['sets'][name]
        got = evaluateNodeClassification(ds['X'].astype(np.float64), ds['Y'], R.TEST_RATIO, seed=R.SPLIT_SEED)
        assert got == (want['micro'], want['macro'], want['accuracy'])
        assert want['default_settings_identical']              # ... which sklearn's default-settings classifier reaches too (the generator's assertion)


def test_determinism_and_expNC(sets):
    ds = sets['std']
    import scipy.sparse as sp
    train = R.train_rows('std', 1024)
    with NC.NodeClassifier(ds['X']) as nc:
        nc.set_labels(sp.csr_matrix(ds['Y']))
        a = nc.fit(train); b = nc.fit(train)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    ratios = [0.3, 0.6]
    e1 = NC.expNC(ds['X'], ds['Y'], ratios, 2, seed=4)
    e2 = NC.expNC(ds['X'], ds['Y'], ratios, 2, seed=4)
    assert e1 == e2 and sorted(e1) == ratios
    for ratio in ratios:
        for r in range(2):
            single = NC.evaluateNodeClassification(ds['X'], ds['Y'], ratio, seed=4 + r)
            assert single == (e1[ratio]['micro'][r], e1[ratio]['macro'][r], e1[ratio]['accuracy'][r])


def refused(code, fragment, fn, *args, **kw):
    with pytest.raises(_hip.GemHipError) as e:
        fn(*args, **kw)
    assert 'error %d:' % code in str(e.value) and fragment in str(e.value), str(e.value)


def test_refusals():
    X = np.arange(12, dtype=np.float32).reshape(6, 2)
    bad = X.copy(); bad[4, 1] = np.nan
    refused(_hip.E_INVALID, 'X[4][1] is not finite', NC.NodeClassifier, bad)
    refused(_hip.E_UNSUPPORTED, 'd = 256', NC.NodeClassifier, np.zeros((2, 256), np.float32))
    Y = np.array([0, 1, 0, 1, 0, 1])
    with NC.NodeClassifier(X) as nc:
        idx = np.arange(6, dtype=np.int32)
        refused(_hip.E_INVALID, 'no labels set', nc.fit, idx)
        refused(_hip.E_INVALID, 'no labels set', nc.predict_topk, idx)
        refused(_hip.E_INVALID, 'entry 2 (row 2) = class 2 outside [0,2)', nc.set_labels, (2, np.arange(7), np.array([0, 1, 2, 1, 0, 1])))
        refused(_hip.E_INVALID, 'entry 1 (row 0) = class -1 outside [0,2)', nc.set_labels, (2, np.array([0, 2, 2, 2, 2, 2, 2]), np.array([0, -1])))
        refused(_hip.E_INVALID, 'entry 1 (row 0) lists class 1 twice', nc.set_labels, (2, np.array([0, 2, 2, 2, 2, 2, 2]), np.array([1, 1])))
        refused(_hip.E_INVALID, 'row_ptr decreases at row 1', nc.set_labels, (2, np.array([0, 2, 1, 2, 2, 2, 2]), np.array([0, 1])))
        refused(_hip.E_INVALID, 'row_ptr[0] = 1', nc.set_labels, (2, np.array([1, 2, 2, 2, 2, 2, 2]), np.array([0, 1])))
        refused(_hip.E_UNSUPPORTED, 'K = 65537', nc.set_labels, (65537, np.arange(7), np.zeros(6, np.int32)))
        nc.set_labels(Y)
        refused(_hip.E_INVALID, 'no weights', nc.predict_topk, idx)
        refused(_hip.E_INVALID, 'no weights', nc.decision_function, idx)
        refused(_hip.E_INVALID, 'row 2 = 6 outside [0,6)', nc.fit, np.array([0, 1, 6, -1], np.int32))
        refused(_hip.E_INVALID, 'row 1 = -1 outside [0,6)', nc.fit, np.array([0, -1], np.int32))
        refused(_hip.E_INVALID, '0 rows', nc.fit, np.zeros(0, np.int32))
        for Cbad in (0.0, -1.0, np.nan, np.inf):
            refused(_hip.E_INVALID, 'C = ', nc.fit, idx, C=Cbad)
        refused(_hip.E_INVALID, 'dec_tol', nc.fit, idx, dec_tol=0.0)
        refused(_hip.E_INVALID, 'max_iter', nc.fit, idx, max_iter=0)
        refused(_hip.E_INVALID, 'the intercept of class 1 is NaN', nc.set_weights, np.array([[0, 0, 0], [0, 0, np.nan]], float))
        refused(_hip.E_INVALID, 'W[0][1] is not finite', nc.set_weights, np.array([[0, np.inf, 0], [0, 0, 0]], float))
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            nc.fit(idx)
        refused(_hip.E_INVALID, 'k[3] = 3 outside [0,2]', nc.predict_topk, idx, np.array([0, 1, 2, 3, 0, 0], np.int32))
        refused(_hip.E_INVALID, 'row 0 = 7 outside [0,6)', nc.predict_topk, np.array([7], np.int32))
        nc.set_labels(Y)                                       # new labels forget the weights
        refused(_hip.E_INVALID, 'no weights', nc.predict_topk, idx)
