"""CPU tier of the t-SNE feature: host logic of gem_amd/evaluation/tsne.py, the plot's default path, the fixtures, and the restatements the GPU
tests lean on (tests/tsne_refs.py) against the sklearn fixtures.  No device call."""
import inspect
import json
import os

import numpy as np
import pytest

import tsne_refs as R
from gem_amd import _hip
from gem_amd.evaluation import tsne


def test_no_host_fallback_without_a_device(monkeypatch):
    monkeypatch.setattr(_hip, 'device_count', lambda: 0)
    X = R.karate_input()
    with pytest.raises(_hip.GemHipError, match='no HIP device'):
        tsne.tsne_2d(X, perplexity=10.0)
    with pytest.raises(_hip.GemHipError, match='no HIP device'):
        tsne.knn(X, 5)
    with pytest.raises(_hip.GemHipError, match='no HIP device'):
        tsne.conditional_affinities(np.ones((3, 8), np.float32), 5.0)
    from gem.evaluation import visualize_embedding as viz
    with pytest.raises(_hip.GemHipError, match='no HIP device'):
        viz.reduce_to_2d(X, reduce='tsne')


def test_pca_init_sign_rule_and_scale():
    rng = np.random.RandomState(5)
    X = rng.standard_normal((200, 7)) * np.array([9.0, 5.0, 1.0, 1.0, 0.5, 0.5, 0.1]) + 3.0
    Y = tsne.pca_init(X)
    assert Y.dtype == np.float32 and Y.shape == (200, 2)
    assert np.std(Y[:, 0].astype(np.float64)) == pytest.approx(1e-4, rel=1e-6)
    Xc = X - X.mean(axis=0)
    _, s, vt = np.linalg.svd(Xc, full_matrices=False)
    for c in range(2):
        v = vt[c] if vt[c][np.argmax(np.abs(vt[c]))] > 0 else -vt[c]             # the component's largest-magnitude entry is positive
        want = Xc @ v / np.std(Xc @ vt[0]) * 1e-4
        assert np.abs(Y[:, c] - want).max() <= 1e-9
    assert np.std(Y[:, 1]) == pytest.approx(1e-4 * s[1] / s[0], rel=1e-5)
    # the rule does not depend on the sign the eigensolver happened to return: a mirrored input gives the mirrored scores' rule again
    Ym = tsne.pca_init(-X)
    assert np.abs(np.abs(Ym) - np.abs(Y)).max() <= 1e-9
    assert tsne.pca_init(X[:, :1]).shape == (200, 2)


def test_learning_rate_auto_and_schedule_constants():
    assert tsne.learning_rate_auto(1024, 12.0) == 50.0
    assert tsne.learning_rate_auto(100000, 12.0) == pytest.approx(100000 / 12.0 / 4.0)
    assert (tsne.EXPLORATION_ITER, tsne.N_ITER_CHECK, tsne.N_ITER_WITHOUT_PROGRESS, tsne.MIN_GRAD_NORM) == (250, 50, 300, 1e-7)
    sig = inspect.signature(tsne.tsne_2d)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [('perplexity', 30.0), ('max_iter', 1000), ('early_exaggeration', 12.0),
                                                                      ('learning_rate', 'auto'), ('init', 'pca'), ('verbose', False)]


def test_plot_default_is_the_pca_projection_it_was():
    from gem.evaluation import visualize_embedding as viz
    assert inspect.signature(viz.plot_embedding2D).parameters['reduce'].default == 'pca'
    X = np.random.RandomState(3).standard_normal((40, 6))
    Xc = X - X.mean(axis=0)
    _, _, vt = np.linalg.svd(Xc, full_matrices=False)
    assert np.array_equal(viz.reduce_to_2d(X), Xc @ vt[:2].T)
    assert np.array_equal(viz.reduce_to_2d(X, reduce='pca'), Xc @ vt[:2].T)
    two = X[:, :2]
    assert np.array_equal(viz.reduce_to_2d(two), two) and np.array_equal(viz.reduce_to_2d(two, reduce='tsne'), two)       # d <= 2: as it is
    with pytest.raises(ValueError):
        viz.reduce_to_2d(X, reduce='umap')
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    plt.figure()
    viz.plot_embedding2D(X, node_colors=np.arange(40))
    pts = plt.gca().collections[0].get_offsets()
    assert np.allclose(np.asarray(pts), Xc @ vt[:2].T, rtol=0, atol=1e-12)
    plt.close('all')


def test_fixtures_load_and_have_the_stated_shapes():
    g = np.load(os.path.join(R.GOLDEN, 'tsne_affinities_ref.npz'))
    for tag, n, k in (('normal', 300, 91), ('karate', 34, 33)):
        ids, dist, P = g[tag + '_id'], g[tag + '_dist'], g[tag + '_P']
        assert ids.shape == dist.shape == P.shape == (n, k)
        assert ids.dtype == np.int32 and dist.dtype == np.float32 and P.dtype == np.float64
        assert np.all(np.diff(dist, axis=1) >= 0) and not np.any(ids == np.arange(n)[:, None])
        assert np.abs(P.sum(axis=1) - 1).max() < 1e-12
    # the inputs are rebuilt, not stored: the stored distances are those of the rebuilt inputs
    for tag, X in (('normal', R.normal_input()), ('karate', R.karate_input())):
        ids, d = R.sorted_knn(R.squared_distances(X), g[tag + '_id'].shape[1])
        assert np.array_equal(d.astype(np.float32), g[tag + '_dist'])
        if tag == 'normal':
            assert np.array_equal(ids, g[tag + '_id'])
    ref = json.load(open(os.path.join(R.GOLDEN, 'tsne_sbm1024_ref.json')))
    assert ref['method'] == 'barnes_hut' and ref['init'] == 'pca' and len(ref['runs']) >= 5
    assert all(1.0 < r['dense_kl'] < 1.5 and 0.9 < r['trustworthiness'] < 1.0 for r in ref['runs'])
    assert R.sbm_input().shape == (1024, 32)


def test_restated_binary_search_is_sklearns():
    """tests/tsne_refs.binary_search_perplexity in fp64 against the fixture: it is the reference of the widths the fixture does not hold."""
    g = np.load(os.path.join(R.GOLDEN, 'tsne_affinities_ref.npz'))
    for tag in ('normal', 'karate'):
        assert np.abs(R.binary_search_perplexity(g[tag + '_dist'], R.PERPLEXITY) - g[tag + '_P']).max() <= 1e-14


def test_restated_gradient_is_the_derivative_of_the_restated_kl():
    """The dense gradient the GPU tests compare with, against central differences of its own KL (exaggeration 1)."""
    g = np.load(os.path.join(R.GOLDEN, 'tsne_affinities_ref.npz'))
    P = R.dense_joint(34, g['karate_id'], g['karate_P'])
    assert P.sum() == pytest.approx(1.0, abs=1e-12) and np.array_equal(P, P.T)
    Y = np.random.RandomState(0).standard_normal((34, 2))
    grad = R.gradient(P, Y, 1.0)[0]
    for i, c in ((0, 0), (5, 1), (33, 0)):
        e = np.zeros_like(Y); e[i, c] = 1e-6
        num = (R.gradient(P, Y + e, 1.0)[1] - R.gradient(P, Y - e, 1.0)[1]) / 2e-6
        assert num == pytest.approx(grad[i, c], rel=1e-5, abs=1e-9)
    assert R.dense_kl(P, Y) == pytest.approx(R.gradient(P, Y, 1.0)[1], rel=1e-12)
