"""Writes the t-SNE fixtures under tests/golden/ (tests/README_tsne.md).  CPU only; needs scikit-learn (1.7.2 when the fixtures were made).

    python scripts/make_golden_tsne.py

tsne_affinities_ref.npz   for (a) seeded N(0,1), n = 300, d = 128 and (b) the karate HOPE embedding (hope_karate_d4.npz, n = 34, d = 4): the
                          k = min(n - 1, 91) smallest squared distances of every row, ascending, float32 (fp64 brute force, rounded once), their ids,
                          and sklearn's _binary_search_perplexity of them at perplexity 30.  Inputs are NOT stored: (a) is normal_input(), (b) an
                          existing golden.
tsne_sbm1024_ref.json     N_RUNS runs of sklearn.manifold.TSNE(n_components=2, init='pca', random_state=s) (default barnes_hut) on
                          hope_sbm1024_d32.npz: each run's KL on the dense fp64 P (_joint_probabilities) and the exact Q, and its trustworthiness
                          at n_neighbors=12."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
PERPLEXITY = 30.0
NORMAL_SEED, NORMAL_N, NORMAL_D = 17, 300, 128            # the seed: see main()
N_RUNS = 5


def normal_input():
    return np.random.RandomState(NORMAL_SEED).standard_normal((NORMAL_N, NORMAL_D)).astype(np.float32)


def karate_input():
    return np.load(os.path.join(GOLDEN, 'hope_karate_d4.npz'))['X'].astype(np.float32)


def sbm_input():
    return np.load(os.path.join(GOLDEN, 'hope_sbm1024_d32.npz'))['X']


def squared_distances(X):
    """fp64, from the differences themselves (no expansion)."""
    X = np.asarray(X, dtype=np.float64)
    D = np.empty((len(X), len(X)))
    for i in range(len(X)):
        D[i] = ((X - X[i]) ** 2).sum(axis=1)
    return D


def knn_bound(X):
    """4 eps32 d max |x - mean|^2: the worst-case rounding of |a|^2 + |b|^2 - 2 a.b in fp32 on the centred rows (tests/README_tsne.md)."""
    X = np.asarray(X, dtype=np.float64)
    return 4.0 * np.finfo(np.float32).eps * X.shape[1] * ((X - X.mean(axis=0)) ** 2).sum(axis=1).max()


def sorted_knn(X, k):
    D = squared_distances(X)
    np.fill_diagonal(D, np.inf)
    ids = np.lexsort((np.broadcast_to(np.arange(len(X)), D.shape), D), axis=1)[:, :k + 1]
    d = np.take_along_axis(D, ids, axis=1)
    return ids[:, :k].astype(np.int32), d[:, :k], d[:, k] - d[:, k - 1] if k + 1 < len(X) else None


def dense_kl(X, Y, perplexity=PERPLEXITY):
    """sklearn's own definition on the dense problem: P from _joint_probabilities on the fp64 squared distances, Q exact, both clamped at
    the fp64 machine epsilon as in _kl_divergence."""
    from scipy.spatial.distance import pdist
    from sklearn.manifold._t_sne import _joint_probabilities
    eps = np.finfo(np.double).eps
    D = squared_distances(X).astype(np.float32)            # TSNE(method='exact') hands float32 distances to _joint_probabilities too
    P = _joint_probabilities(D, perplexity, 0).astype(np.float64)
    q = 1.0 / (1.0 + pdist(np.asarray(Y, dtype=np.float64), 'sqeuclidean'))
    Q = np.maximum(q / (2.0 * q.sum()), eps)
    return float(2.0 * np.dot(P, np.log(np.maximum(P, eps) / Q)))


def main():
    from sklearn.manifold import TSNE, trustworthiness
    from sklearn.manifold._utils import _binary_search_perplexity
    import sklearn
    out = {}
    for tag, X in (('normal', normal_input()), ('karate', karate_input())):
        n = len(X)
        k = min(n - 1, int(3.0 * PERPLEXITY + 1))
        ids, d64, gap = sorted_knn(X, k)
        d32 = d64.astype(np.float32)
        P = _binary_search_perplexity(np.ascontiguousarray(d32), PERPLEXITY, 0)
        assert P.dtype == np.float64 and P.shape == (n, k) and np.all(np.abs(P.sum(axis=1) - 1) < 1e-12)
        out[tag + '_id'] = ids; out[tag + '_dist'] = d32; out[tag + '_P'] = P
        bound = knn_bound(X)
        print('%s: n = %d, d = %d, k = %d, kNN bound %.3e, smallest gap at rank k %s' % (tag, n, X.shape[1], k, bound, 'none (k = n - 1)' if gap is None else '%.3e' % gap.min()))
        if tag == 'normal':
            # The GPU test demands numpy's id sets exactly on this input.  No seed gives a smallest gap (over 300 rows, mean gap 0.16) above twice
            # the WORST-CASE bound (1.1e-2): of seeds 0..39, 17 has the largest, 3.6e-3.  What is asserted is the gap against twice the bound with
            # sqrt(d) in the place of d -- rounding errors of a d-term sum adding like a random walk -- which is what the exact-set check rests on.
            assert gap.min() > 2.0 * bound / np.sqrt(X.shape[1]), (gap.min(), bound)
    np.savez_compressed(os.path.join(GOLDEN, 'tsne_affinities_ref.npz'), **out)

    X = sbm_input()
    runs = []
    for seed in range(N_RUNS):
        Y = TSNE(n_components=2, init='pca', random_state=seed).fit_transform(X)
        runs.append({'seed': seed, 'dense_kl': dense_kl(X, Y), 'trustworthiness': float(trustworthiness(X, Y, n_neighbors=12))})
        print(runs[-1], flush=True)
    with open(os.path.join(GOLDEN, 'tsne_sbm1024_ref.json'), 'w') as fh:
        json.dump({'input': 'hope_sbm1024_d32.npz:X', 'perplexity': PERPLEXITY, 'sklearn': sklearn.__version__, 'method': 'barnes_hut', 'init': 'pca',
                   'trustworthiness_n_neighbors': 12, 'runs': runs}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    sys.exit(main())
