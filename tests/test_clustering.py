"""CPU tier of clustering (tests/README_clustering.md): the host scores against sklearn.metrics, the restatements against the sklearn
fixture, the relocation order, the host refusals, and the refusal of every device entry without a device."""
import ctypes as C
import json

import numpy as np
import pytest

import clustering_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import clustering as CL


@pytest.fixture(scope='module')
def fixture():
    return json.load(open(golden_path('clustering_ref.json'))), np.load(golden_path('clustering_ref.npz'))


def check_against_sklearn(pred, true):
    from sklearn.metrics import adjusted_rand_score, homogeneity_score, normalized_mutual_info_score
    Kp, Kt = int(pred.max()) + 1, int(true.max()) + 1
    table = R.contingency_ref(pred, true, Kp, Kt)
    nmi, ari, purity, hom = CL.clustering_scores(table)
    assert nmi == pytest.approx(normalized_mutual_info_score(true, pred), abs=1e-12)
    assert ari == pytest.approx(adjusted_rand_score(true, pred), abs=1e-12)
    assert hom == pytest.approx(homogeneity_score(true, pred), abs=1e-12)
    ref = R.scores_ref(table)
    assert (nmi, ari, purity) == pytest.approx(ref, abs=1e-12)
    return nmi, ari, purity


def test_scores_against_sklearn_on_the_fixture_tables(fixture):
    meta, arr = fixture
    lt = R.sbm_labels()
    seen = 0
    for name, entry in meta['sets'].items():
        if 'scores' not in entry:
            continue
        nmi, ari, purity = check_against_sklearn(arr['labels_%s_tol1e-4' % name], lt)
        want = entry['scores']
        assert (nmi, ari, purity) == pytest.approx((want['nmi'], want['ari'], want['purity']), abs=1e-12)
        assert CL.clustering_scores(want['table'])[:3] == (nmi, ari, purity)
        seen += 1
    assert seen == 3
    assert meta['sets']['sbm_k3_s1']['scores']['nmi'] == 1.0 and meta['sets']['sbm_k3_s1']['scores']['ari'] == 1.0


def test_scores_special_partitions():
    rng = np.random.RandomState(0)
    true = rng.randint(0, 5, size=400)
    perm = np.array([3, 0, 4, 1, 2])
    assert check_against_sklearn(perm[true], true) == (pytest.approx(1.0, abs=1e-12), 1.0, 1.0)       # a perfect match under a permutation of ids
    nmi, ari, purity = check_against_sklearn(np.zeros(400, np.int64), true)                          # one cluster against many
    assert nmi == 0.0 and ari == 0.0 and purity == np.bincount(true).max() / 400.0
    assert check_against_sklearn(np.zeros(7, np.int64), np.zeros(7, np.int64)) == (1.0, 1.0, 1.0)     # both a single cluster
    nmi, ari, _ = check_against_sklearn(rng.randint(0, 4, size=400), true)                           # independent partitions
    assert 0.0 <= nmi < 0.05 and abs(ari) < 0.05


def test_scores_with_empty_rows_and_columns():
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    table = np.array([[5, 0, 2, 0], [0, 0, 0, 0], [1, 0, 7, 0], [0, 0, 0, 0], [3, 0, 3, 0]], np.int64)
    pred = np.repeat(np.arange(5), table.sum(axis=1)); true = np.concatenate([np.repeat(np.arange(4), row) for row in table])
    nmi, ari, purity, _ = CL.clustering_scores(table)
    assert nmi == pytest.approx(normalized_mutual_info_score(true, pred), abs=1e-12)
    assert ari == pytest.approx(adjusted_rand_score(true, pred), abs=1e-12)
    assert purity == (5 + 7 + 3) / 21.0
    dense = table[[0, 2, 4]][:, [0, 2]]
    assert CL.clustering_scores(dense)[:3] == (nmi, ari, purity)


def test_ari_does_not_overflow():
    """n = 10^6 rows against sklearn (its pair counts pass 2^39), and a table of 2^31 - 1 rows against Python integers: n^2 and the products
    of two pair counts need more than 64 bits."""
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    rng = np.random.RandomState(1)
    true = rng.randint(0, 10, size=1000000)
    pred = np.where(rng.rand(1000000) < 0.8, true, rng.randint(0, 10, size=1000000))
    table = R.contingency_ref(pred, true, 10, 10)
    nmi, ari, _, _ = CL.clustering_scores(table)
    assert ari == pytest.approx(adjusted_rand_score(true, pred), abs=1e-12)
    assert nmi == pytest.approx(normalized_mutual_info_score(true, pred), abs=1e-12)
    big = np.array([[900000000, 100000000, 3], [50000000, 800000000, 0], [0, 97483644, 200000000]], np.int64)
    assert big.sum() == 2 ** 31 - 1
    assert CL.clustering_scores(big)[:3] == pytest.approx(R.scores_ref(big), abs=1e-12)
    assert 0.3 < CL.clustering_scores(big)[1] < 1.0


def test_purity_by_hand():
    table = [[4, 1, 0], [2, 2, 6], [0, 3, 0]]
    assert CL.clustering_scores(table)[2] == (4 + 6 + 3) / 18.0
    assert CL.clustering_scores([[3, 3]])[2] == 0.5                     # a tie is one majority
    assert CL.clustering_scores([[1, 0], [0, 1]])[:3] == (pytest.approx(1.0, abs=1e-15), 1.0, 1.0)


def test_scores_refusals():
    L = _hip.lib()
    out = (C.c_double * 4)()
    t = np.array([[1, -2], [3, 4]], np.int64)
    assert L.gemhip_clustering_scores_host(_hip.ptr(t, C.c_int64), 2, 2, out) == _hip.E_INVALID
    assert L.gemhip_last_error() == b'clustering_scores_host: table[0][1] = -2 is negative'
    z = np.zeros((2, 3), np.int64)
    assert L.gemhip_clustering_scores_host(_hip.ptr(z, C.c_int64), 2, 3, out) == _hip.E_INVALID and b'empty' in L.gemhip_last_error()
    assert L.gemhip_clustering_scores_host(_hip.ptr(z, C.c_int64), 0, 3, out) == _hip.E_INVALID
    assert L.gemhip_clustering_scores_host(None, 2, 3, out) == _hip.E_INVALID
    with pytest.raises(ValueError):
        CL.clustering_scores(np.zeros(3, np.int64))
    with pytest.raises(_hip.GemHipError):
        CL.clustering_scores(z)


def test_restated_lloyd_equals_the_fixture(fixture):
    meta, arr = fixture
    sets = R.data_sets()
    assert sorted(sets) == sorted(meta['sets'])
    for name, ds in sets.items():
        for tag, tol in (('tol0', 0.0), ('tol1e-4', 1e-4)):
            want = meta['sets'][name][tag]
            ref = R.lloyd(ds['X'], ds['C0'], tol=tol)
            assert np.array_equal(ref['labels'], arr['labels_%s_%s' % (name, tag)]) and ref['n_iter'] == want['n_iter'], (name, tag)
            assert ref['strict'] == want['strict'] and ref['tight'] == 0
            c32 = arr['centres_%s_%s' % (name, tag)].astype(np.float32)
            assert np.all(np.abs(c32.astype(np.float64) - ref['centres']) <= np.spacing(np.abs(c32))), (name, tag)
            assert ref['inertia'] == pytest.approx(want['inertia'], rel=1e-9)
            assert [[it, rows] for it, rows in ref['relocated']] == want['relocated']
            assert bool(ref['relocated']) == (name in R.RELOCATION_SETS)


def test_restated_seeding_equals_the_fixture(fixture):
    meta, arr = fixture
    for name, ds in R.seed_sets().items():
        rows, margin = R.seed_pp_ref(ds['X'], ds['K'], ds['u'])
        assert np.array_equal(rows, arr['seed_rows_%s' % name]) and margin >= 1e-5
        assert meta['seeding'][name]['margin'] >= 1e-5
    assert CL.default_trials(100) == 6 and CL.default_trials(3) == 3 and CL.default_trials(1) == 2
    assert np.array_equal(CL.seed_uniforms(13, 2, 4), np.random.RandomState(2).uniform(size=(13, 4)))


def test_relocation_order_on_equal_distances():
    """Six rows on a line around two live centres, two empty clusters: rows 1 and 4 are the farthest and equally far (distance 9), so the
    lower row id goes to the lower empty cluster; row 4's donor keeps its other rows."""
    X = np.array([[0.0], [-3.0], [1.0], [10.0], [13.0], [9.0]], np.float32)
    C_old = np.array([[0.0], [50.0], [10.0], [60.0]], np.float32)
    labels = R.assign_ref(X, C_old)[0]
    assert labels.tolist() == [0, 0, 0, 2, 2, 2]
    _, counts, sums = R.update_ref(X, labels, 4)
    rows = R.relocate_ref(X, C_old, labels, sums, counts)
    assert rows == [1, 4]
    assert counts.tolist() == [2, 1, 2, 1]
    assert R.centres_of(sums, counts).ravel().tolist() == [0.5, -3.0, 9.5, 13.0]
    with pytest.raises(ValueError, match='without a row'):                 # the farthest row is alone in its cluster
        Xs = np.array([[0.0], [1.0], [100.0]], np.float32); Cs = np.array([[0.5], [90.0], [-500.0]], np.float32)
        lab = R.assign_ref(Xs, Cs)[0]
        _, cnt, sm = R.update_ref(Xs, lab, 3)
        R.relocate_ref(Xs, Cs, lab, sm, cnt)


def test_fixtures_load_with_the_stated_shapes(fixture):
    meta, arr = fixture
    assert meta['sklearn'] == '1.7.2'
    for name, ds in R.data_sets().items():
        e = meta['sets'][name]
        assert (e['n'], e['d'], e['K']) == (ds['X'].shape[0], ds['X'].shape[1], ds['K'])
        for tag in ('tol0', 'tol1e-4'):
            assert arr['labels_%s_%s' % (name, tag)].shape == (e['n'],) and arr['labels_%s_%s' % (name, tag)].dtype == np.int32
            assert arr['centres_%s_%s' % (name, tag)].shape == (e['K'], e['d']) and arr['centres_%s_%s' % (name, tag)].dtype == np.float64
    want = {'prime_k8_s1': 14, 'prime_k8_s2': 14, 'prime_k13_s0': 13, 'prime_k13_s2': 13, 'normal_k5_s3': 12, 'sbm_k3_s1': 5, 'sbm_k3_s3': 36, 'sbm_k7_s1': 20}
    assert {k: v['tol0']['n_iter'] for k, v in meta['sets'].items()} == want
    for name, ds in R.seed_sets().items():
        assert arr['seed_rows_%s' % name].shape == (ds['K'],)


def test_l2_normalize_keeps_zero_rows():
    X = np.array([[3.0, 4.0], [0.0, 0.0], [1e-20, 0.0]], np.float32)
    Y = CL.l2_normalize(X)
    assert Y.dtype == np.float32 and Y[0].tolist() == [np.float32(0.6), np.float32(0.8)] and Y[1].tolist() == [0.0, 0.0] and Y[2].tolist() == [1.0, 0.0]


def test_every_device_entry_refuses_without_a_device():
    from gem_amd import evaluation
    assert evaluation.evaluateClustering is CL.evaluateClustering and evaluation.KMeans is CL.KMeans
    if _hip.device_count() > 0:
        pytest.skip('GPU present')
    X = np.zeros((4, 2), np.float32)
    with pytest.raises(_hip.GemHipError):
        CL.KMeans(X)
    with pytest.raises(_hip.GemHipError):
        CL.evaluateClustering(X, np.array([0, 1, 0, 1]))
    with pytest.raises(_hip.GemHipError):
        CL.expClustering(X, np.array([0, 1, 0, 1]), 1)


def test_create_refuses_bad_input_on_the_host():
    """gemhip_kmeans_create checks everything before its first device call, so these run without a GPU."""
    L = _hip.lib()
    h = C.c_void_p()

    def create(n, d, ld, X):
        return L.gemhip_kmeans_create(n, d, ld, _hip.ptr(X, C.c_float), C.byref(h))
    X = np.zeros((5, 6), np.float32)
    for bad, where in ((np.nan, (3, 2)), (np.inf, (0, 0)), (-np.inf, (4, 3))):
        Y = X.copy(); Y[where] = bad; Y[4, 5] = np.nan                    # the last column is padding at d = 4 .. 5
        assert create(5, 5, 6, Y) == _hip.E_INVALID
        assert L.gemhip_last_error() == b'kmeans_create: X[%d][%d] is not finite' % where
    assert create(5, 0, 6, X) == _hip.E_INVALID and create(5, 7, 6, X) == _hip.E_INVALID and create(0, 4, 6, X) == _hip.E_INVALID
    assert create(5, 4, 6, None) == _hip.E_INVALID
    assert create(2 ** 31, 4, 6, X) == _hip.E_UNSUPPORTED and b'below 2^31' in L.gemhip_last_error()
    assert create(5, 257, 300, X) == _hip.E_UNSUPPORTED and b'at most 256' in L.gemhip_last_error()
    assert not h.value
