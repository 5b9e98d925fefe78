"""GPU tier of clustering (tests/README_clustering.md): gem_amd/csrc/kmeans.hip stage by stage and end to end against the restatements of
tests/clustering_refs.py and the sklearn fixture.  Every tolerance is a derived bound; the measured fractions are printed (-s)."""
import ctypes as C
import json
import warnings

import numpy as np
import pytest

import clustering_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import clustering as CL

pytestmark = pytest.mark.gpu

ROWS, TILE, MAX_D, MAX_K, MAX_TRIALS, SLICE = 128, 32, 256, 16384, 16, 512


@pytest.fixture(scope='module')
def fixture():
    return json.load(open(golden_path('clustering_ref.json'))), np.load(golden_path('clustering_ref.npz'))


@pytest.fixture(scope='module')
def sets():
    return R.data_sets()


def padded(X, pad=3):
    """X with `pad` NaN columns behind it: the device must never read them."""
    out = np.full((X.shape[0], X.shape[1] + pad), np.nan, np.float32)
    out[:, :X.shape[1]] = X
    return out


def test_constants_read_back():
    """The shapes below are chosen around these."""
    with CL.KMeans(np.zeros((300, 5), np.float32)) as km:
        s = km.stats()
    assert (s['assign_rows'], s['centre_tile'], s['max_d'], s['max_K'], s['max_trials'], s['slice_members']) == (ROWS, TILE, MAX_D, MAX_K, MAX_TRIALS, SLICE)
    assert (s['n'], s['d'], s['d_padded'], s['K'], s['slab_rows']) == (300, 5, 8, 0, 256)


def check_assign(X, Cn, tag):
    n, d = X.shape
    K = len(Cn)
    with CL.KMeans(padded(X), d=d) as km:
        labels, score = km.assign(K, Cn, want_score=True)
    ref, s64, gap, B = R.assign_ref(X, Cn)
    assert labels.min() >= 0 and labels.max() < K
    clear = gap > 2 * B
    assert np.array_equal(labels[clear], ref[clear]), tag
    chosen = s64[np.arange(n), labels]
    assert np.all(chosen - s64.min(axis=1) <= 2 * B), tag
    assert np.all(np.abs(score.astype(np.float64) - chosen) <= B), tag
    share = float((~clear).mean())
    assert share <= 0.01, (tag, share)                        # the reference's own share of undecidable rows
    assert float((labels != ref).mean()) <= 0.01, tag
    print('assign %s: tight rows %d of %d, labels off the fp64 arg-min %d, worst score error %.3f B'
          % (tag, int((~clear).sum()), n, int((labels != ref).sum()), float((np.abs(score - chosen) / B).max())))


@pytest.mark.parametrize('d', [1, 2, 32, 33, 128, 131])
def test_assign_every_width(d):
    rng = np.random.RandomState(d)
    check_assign(rng.standard_normal((1061, d)).astype(np.float32), rng.standard_normal((TILE + 1, d)).astype(np.float32), 'd=%d' % d)


@pytest.mark.parametrize('n', [1, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 1061])
def test_assign_every_row_count(n):
    rng = np.random.RandomState(n)
    check_assign(rng.standard_normal((n, 33)).astype(np.float32), rng.standard_normal((min(n, 5), 33)).astype(np.float32), 'n=%d' % n)


@pytest.mark.parametrize('K', [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 200])
def test_assign_every_centre_count(K):
    rng = np.random.RandomState(K)
    X = rng.standard_normal((200, 33)).astype(np.float32)
    check_assign(X, X.copy() if K == 200 else rng.standard_normal((K, 33)).astype(np.float32), 'K=%d' % K)       # K = n: every row its own centre


def test_assign_tie_rule():
    """Small integers: every fp32 product and sum is exact, so equal scores are equal on the device too and the label is the restatement's --
    the lower id.  Centres 33 .. 40 repeat centres 2 .. 9 (a tile apart), centres 0 and 1 mirror each other (every row with x_0 = 0 is
    equidistant), rows repeat."""
    rng = np.random.RandomState(7)
    X = rng.randint(-3, 4, size=(300, 5)).astype(np.float32)
    X[::3, 0] = 0
    X[150:] = X[:150]
    Cn = rng.randint(-3, 4, size=(41, 5)).astype(np.float32)
    Cn[0] = [2, 0, 0, 0, 0]; Cn[1] = [-2, 0, 0, 0, 0]; Cn[33:41] = Cn[2:10]
    with CL.KMeans(X) as km:
        labels = km.assign(41, Cn)
    ref, s64, gap, _ = R.assign_ref(X, Cn)
    assert np.array_equal(labels, ref)
    assert (gap == 0).sum() > 20 and not np.any(labels >= 33)
    print('tie rule: %d of 300 rows have two equal best scores' % int((gap == 0).sum()))


def update_tolerance(X, labels, K):
    X64 = np.abs(np.asarray(X, dtype=np.float64))
    counts = np.bincount(labels, minlength=K)
    absum = np.zeros((K, X.shape[1]))
    np.add.at(absum, labels, X64)
    return 2.0 ** -50 * absum / np.maximum(counts, 1)[:, None]


def check_centres(Cdev, Cref32, X, labels, K, tag):
    """Within one fp32 ulp of float32(fp64 mean) plus 2^-50 sum |x| / count."""
    err = np.abs(Cdev.astype(np.float64) - Cref32.astype(np.float64))
    bound = np.spacing(np.abs(Cref32)).astype(np.float64) + update_tolerance(X, labels, K)
    assert np.all(err <= bound), (tag, float((err / bound).max()))
    print('centres %s: %d of %d entries differ from float32(fp64 mean), worst %.3f of the bound' % (tag, int((err > 0).sum()), err.size, float((err / bound).max())))


def test_update():
    X = R.inputs()['prime']
    n = len(X)
    rng = np.random.RandomState(3)
    one_row = rng.randint(0, 6, size=n); one_row[one_row == 4] = 0; one_row[517] = 4           # cluster 4 holds one row
    cases = {'random K=7': (7, rng.randint(0, 7, size=n)), 'one row': (6, one_row), 'all rows in one of three': (3, np.full(n, 1)),
             'K=1': (1, np.zeros(n, np.int64)), 'K=n': (n, rng.permutation(n))}
    with CL.KMeans(padded(X), d=X.shape[1]) as km:
        for tag, (K, labels) in cases.items():
            Cdev, counts = km.update(K, labels)
            Cref, cref, _ = R.update_ref(X, labels.astype(np.int64), K)
            assert np.array_equal(counts, cref), tag
            assert np.all(Cdev[cref == 0] == 0), tag
            check_centres(Cdev, Cref, X, labels, K, tag)
            assert np.array_equal(km.contingency(np.zeros(n, np.int32))[:, 0], cref), tag        # the labels stayed on the device
        again = km.update(7, cases['random K=7'][1])[0]
        assert np.array_equal(again, km.update(7, cases['random K=7'][1])[0])


@pytest.mark.parametrize('name', R.RELOCATION_SETS)
def test_relocation_on_the_prime_sets(name, sets, fixture):
    """Both sets lose clusters in their second iteration: the centres after it match the restatement's."""
    ds = sets[name]
    want = fixture[0]['sets'][name]['tol0']['relocated']
    ref = R.lloyd(ds['X'], ds['C0'], tol=0.0, max_iter=2)
    assert [[it, rows] for it, rows in ref['relocated']] == want
    with CL.KMeans(ds['X']) as km:
        labels, Cdev, info = km.fit(ds['K'], init=ds['C0'], tol=0.0, max_iter=2, warn=False)
    assert info['relocations'] == len(want[0][1]) and info['iterations'] == 2 and not info['strict']
    assert np.array_equal(labels, ref['labels'])
    err = np.abs(Cdev.astype(np.float64) - ref['centres'])
    assert np.all(err <= np.spacing(np.abs(ref['centres'])) + update_tolerance(ds['X'], ref['labels'], ds['K'])), name
    for row in want[0][1]:                                               # a relocated cluster's centre is the row itself
        assert np.any(np.all(Cdev == ds['X'][row], axis=1))


def test_relocation_order_on_equal_distances():
    """The built case of tests/test_clustering.py: two empty clusters, rows 1 and 4 equally far; and the refusal when the donor would be emptied."""
    X = np.array([[0.0], [-3.0], [1.0], [10.0], [13.0], [9.0]], np.float32)
    C_old = np.array([[0.0], [50.0], [10.0], [60.0]], np.float32)
    with CL.KMeans(X) as km:
        labels, Cdev, info = km.fit(4, init=C_old, tol=0.0, max_iter=1, warn=False)
    assert Cdev.ravel().tolist() == [0.5, -3.0, 9.5, 13.0] and info['relocations'] == 2
    assert labels.tolist() == [0, 1, 0, 2, 3, 2]                         # the extra assign of a non-strict stop
    Xs = np.array([[0.0], [1.0], [100.0]], np.float32); Cs = np.array([[0.5], [90.0], [-500.0]], np.float32)
    with CL.KMeans(Xs) as km:
        with pytest.raises(_hip.GemHipError, match=r'error -3: kmeans fit: moving row 2 into the empty cluster 2 would leave its cluster 1 without a row'):
            km.fit(3, init=Cs, max_iter=5)


@pytest.mark.parametrize('name', [s[0] for s in R.FIT_SETS])
def test_fit_equals_the_fixture(name, sets, fixture):
    meta, arr = fixture
    ds = sets[name]
    X, K = ds['X'], ds['K']
    with CL.KMeans(padded(X), d=X.shape[1]) as km:
        for tag, tol in (('tol0', 0.0), ('tol1e-4', 1e-4)):
            want = meta['sets'][name][tag]
            labels, Cdev, info = km.fit(K, init=ds['C0'], tol=tol)
            assert np.array_equal(labels, arr['labels_%s_%s' % (name, tag)]) and info['iterations'] == want['n_iter'], (name, tag)
            assert info['strict'] == want['strict'] and info['converged']
            assert info['relocations'] == sum(len(rows) for _, rows in want['relocated'])
            check_centres(Cdev, arr['centres_%s_%s' % (name, tag)].astype(np.float32), X, labels, K, '%s %s' % (name, tag))
            assert info['inertia'] == pytest.approx(want['inertia'], rel=1e-6)
            print('fit %s %s: %d iterations, inertia off by %.1e' % (name, tag, info['iterations'], abs(info['inertia'] / want['inertia'] - 1)))
        with pytest.warns(RuntimeWarning, match='not converged after max_iter = 2'):
            labels, Cdev, info = km.fit(K, init=ds['C0'], tol=0.0, max_iter=2)
        assert info['iterations'] == 2 and not info['converged']
        ref, _, gap, B = R.assign_ref(X, Cdev)                           # the labels belong to the returned centres
        assert np.array_equal(labels[gap > 2 * B], ref[gap > 2 * B])
        assert info['inertia'] == pytest.approx(R.inertia_ref(X, Cdev, labels), rel=1e-12)


def test_seed_pp(fixture):
    arr = fixture[1]
    for name, ds in R.seed_sets().items():
        with CL.KMeans(padded(ds['X']), d=ds['X'].shape[1]) as km:
            rows, Cdev = km.seed_pp(ds['K'], u=ds['u'])
        assert np.array_equal(rows, arr['seed_rows_%s' % name]), name
        assert len(set(rows.tolist())) == ds['K'] and np.array_equal(Cdev, ds['X'][rows])
    X = R.inputs()['normal'][:40]
    with CL.KMeans(X) as km:
        rows, _ = km.seed_pp(40, seed=5)                                 # K = n: every row once
        assert sorted(rows.tolist()) == list(range(40))
        first = km.seed_pp(3, u=np.array([[0.999999999], [0.0], [0.5]]))[0]
        assert first[0] == 39 and first[1] != 39
        assert np.array_equal(km.seed_pp(7, seed=1)[0], km.seed_pp(7, seed=1)[0])


def test_contingency_and_end_to_end(sets, fixture):
    meta, arr = fixture
    lt = R.sbm_labels()
    for name in ('sbm_k3_s1', 'sbm_k3_s3'):
        ds = sets[name]
        want = meta['sets'][name]['scores']
        nmi, ari, purity, inertia, labels = CL.evaluateClustering(ds['X'], lt, init=ds['C0'], return_labels=True)
        assert np.array_equal(labels, arr['labels_%s_tol1e-4' % name])
        assert (nmi, ari, purity) == pytest.approx((want['nmi'], want['ari'], want['purity']), abs=1e-12)
        assert inertia == pytest.approx(meta['sets'][name]['tol1e-4']['inertia'], rel=1e-6)
        with CL.KMeans(ds['X']) as km:
            labels = km.fit(3, init=ds['C0'])[0]
            table = km.contingency(lt)
            assert np.array_equal(table, R.contingency_ref(labels, lt, 3, 3)) and table.tolist() == want['table']
            assert np.array_equal(km.contingency(lt, n_classes=5)[:, :3], table)
    X = sets['sbm_k3_s1']['X']
    assert CL.evaluateClustering(X, lt, seed=4)[:3] == pytest.approx((1.0, 1.0, 1.0), abs=1e-12)      # k-means++ finds the three blocks
    # normalize='l2' is the fit of the pre-normalised matrix; zero rows stay zero
    Xz = X.copy(); Xz[5] = 0
    a = CL.evaluateClustering(Xz, lt, seed=2, normalize='l2', return_labels=True)
    b = CL.evaluateClustering(CL.l2_normalize(Xz), lt, seed=2, return_labels=True)
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
    # n_init = 3 keeps the best of its three runs, and the device's labels are that run's
    Xp = sets['prime_k8_s1']['X']
    with CL.KMeans(Xp) as km:
        singles = [km.fit(8, seed=10 + r) for r in range(3)]
        labels, Cdev, info = km.fit(8, seed=10, n_init=3)
        best = int(np.argmin([s[2]['inertia'] for s in singles]))
        assert info['run'] == best and info['inertia'] == singles[best][2]['inertia']
        assert np.array_equal(labels, singles[best][0]) and np.array_equal(Cdev, singles[best][1])
        assert np.array_equal(km.contingency(np.zeros(len(Xp), np.int32))[:, 0], np.bincount(labels, minlength=8))


def test_determinism_and_expClustering(sets):
    ds = sets['sbm_k7_s1']
    lt = R.sbm_labels()
    with CL.KMeans(ds['X']) as km:
        a = km.fit(7, seed=3)
        b = km.fit(7, seed=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]['inertia'] == b[2]['inertia'] and a[2]['iterations'] == b[2]['iterations']
    e1 = CL.expClustering(ds['X'], lt, 2, seed=6, n_clusters=7)
    e2 = CL.expClustering(ds['X'], lt, 2, seed=6, n_clusters=7)
    assert e1 == e2
    for r in range(2):
        single = CL.evaluateClustering(ds['X'], lt, n_clusters=7, seed=6 + r)
        assert (e1['nmi'][r], e1['ari'][r], e1['purity'][r], e1['inertia'][r]) == single
    assert e1['mean']['nmi'] == float(np.mean(e1['nmi']))


def test_refusals():
    L = _hip.lib()
    X = np.random.RandomState(0).standard_normal((50, 4)).astype(np.float32)
    Cn = X[:3].copy()
    labels = np.zeros(50, np.int32); out_c = np.zeros((3, 4), np.float32); cnt = np.zeros(3, np.int64); info = np.zeros(6)
    rows = np.zeros(3, np.int32); table = np.zeros((3, 3), np.int64)

    def err(rc, code, text):
        assert rc == code and text in L.gemhip_last_error(), (rc, L.gemhip_last_error())

    def fp(a):
        return _hip.ptr(a, C.c_float)

    def ip(a):
        return _hip.ptr(a, C.c_int32)
    with CL.KMeans(X) as km:
        h = km._h
        err(L.gemhip_kmeans_contingency(h, 3, ip(labels), _hip.ptr(table, C.c_int64)), _hip.E_INVALID, b'no labels on the device')
        for K, code, text in ((0, _hip.E_INVALID, b'K = 0'), (-1, _hip.E_INVALID, b'K = -1'), (51, _hip.E_INVALID, b'K = 51 exceeds n = 50')):
            err(L.gemhip_kmeans_fit(h, K, fp(Cn), 1e-4, 10, ip(labels), _hip.ptr(info, C.c_double)), code, text)
            err(L.gemhip_kmeans_assign(h, K, fp(Cn), ip(labels), None), code, text)
            err(L.gemhip_kmeans_update(h, K, ip(labels), fp(out_c), _hip.ptr(cnt, C.c_int64)), code, text)
            err(L.gemhip_kmeans_seed_pp(h, K, 1, _hip.ptr(np.zeros((3, 1)), C.c_double), ip(rows), fp(out_c)), code, text)
        bad = Cn.copy(); bad[2, 1] = np.inf
        err(L.gemhip_kmeans_fit(h, 3, fp(bad), 1e-4, 10, ip(labels), None), _hip.E_INVALID, b'kmeans_fit: centre[2][1] is not finite')
        err(L.gemhip_kmeans_assign(h, 3, fp(bad), ip(labels), None), _hip.E_INVALID, b'kmeans_assign: centre[2][1] is not finite')
        err(L.gemhip_kmeans_fit(h, 3, fp(Cn), 1e-4, 0, ip(labels), None), _hip.E_INVALID, b'max_iter = 0')
        for tol in (-1e-9, float('nan'), float('inf')):
            err(L.gemhip_kmeans_fit(h, 3, fp(Cn), tol, 10, ip(labels), None), _hip.E_INVALID, b'kmeans_fit: tol')
        u = np.full((3, 2), 0.5); u[1, 1] = 1.0
        err(L.gemhip_kmeans_seed_pp(h, 3, 2, _hip.ptr(u, C.c_double), ip(rows), fp(out_c)), _hip.E_INVALID, b'u[1][1] = 1 outside [0,1)')
        u[1, 1] = -0.25
        err(L.gemhip_kmeans_seed_pp(h, 3, 2, _hip.ptr(u, C.c_double), ip(rows), fp(out_c)), _hip.E_INVALID, b'u[1][1] = -0.25 outside [0,1)')
        u[1, 1] = np.nan
        err(L.gemhip_kmeans_seed_pp(h, 3, 2, _hip.ptr(u, C.c_double), ip(rows), fp(out_c)), _hip.E_INVALID, b'u[1][1]')
        err(L.gemhip_kmeans_seed_pp(h, 3, 0, _hip.ptr(u, C.c_double), ip(rows), fp(out_c)), _hip.E_INVALID, b'n_trials = 0')
        err(L.gemhip_kmeans_seed_pp(h, 3, MAX_TRIALS + 1, _hip.ptr(np.zeros((3, MAX_TRIALS + 1)), C.c_double), ip(rows), fp(out_c)), _hip.E_UNSUPPORTED,
            b'at most 16')
        lab = labels.copy(); lab[17] = 3
        err(L.gemhip_kmeans_update(h, 3, ip(lab), fp(out_c), _hip.ptr(cnt, C.c_int64)), _hip.E_INVALID, b'label 17 = 3 outside [0,3)')
        lab[17] = -1
        err(L.gemhip_kmeans_update(h, 3, ip(lab), fp(out_c), _hip.ptr(cnt, C.c_int64)), _hip.E_INVALID, b'label 17 = -1 outside [0,3)')
        km.assign(3, Cn)
        err(L.gemhip_kmeans_contingency(h, 3, ip(lab), _hip.ptr(table, C.c_int64)), _hip.E_INVALID, b'true label 17 = -1 outside [0,3)')
        lab[17] = 3
        err(L.gemhip_kmeans_contingency(h, 3, ip(lab), _hip.ptr(table, C.c_int64)), _hip.E_INVALID, b'true label 17 = 3 outside [0,3)')
        err(L.gemhip_kmeans_contingency(h, 0, ip(labels), _hip.ptr(table, C.c_int64)), _hip.E_INVALID, b'Kt = 0')
        with pytest.raises(ValueError):
            km.fit(3, init='random')
        with pytest.raises(ValueError):
            km.fit(3, init=Cn[:2])
    with CL.KMeans(np.zeros((MAX_K + 2, 1), np.float32)) as km:
        big = np.zeros((MAX_K + 1, 1), np.float32); lab = np.zeros(MAX_K + 2, np.int32)
        err(L.gemhip_kmeans_assign(km._h, MAX_K + 1, fp(big), ip(lab), None), _hip.E_UNSUPPORTED, b'at most 16384 clusters')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        with CL.KMeans(X) as km:                                         # a converged fit warns nothing
            km.fit(3, seed=0)
