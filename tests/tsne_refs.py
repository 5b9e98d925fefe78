"""Host restatements the t-SNE tests compare gem_amd/csrc/tsne.hip with (tests/README_tsne.md).  numpy only; `dtype` selects the precision
every step is carried out in, so the same function is the fp64 reference and the fp32 yardstick."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
PERPLEXITY = 30.0
NORMAL_SEED, NORMAL_N, NORMAL_D = 17, 300, 128                # scripts/make_golden_tsne.py
MACHINE_EPS = np.finfo(np.double).eps


def normal_input():
    return np.random.RandomState(NORMAL_SEED).standard_normal((NORMAL_N, NORMAL_D)).astype(np.float32)


def karate_input():
    return np.load(os.path.join(GOLDEN, 'hope_karate_d4.npz'))['X'].astype(np.float32)


def sbm_input():
    return np.load(os.path.join(GOLDEN, 'hope_sbm1024_d32.npz'))['X']


def prime_input():
    """n = 1061 (prime), d = 33 (odd): ragged row blocks, ragged j-slices, an unaligned row stride.  Eight loose clusters."""
    rng = np.random.RandomState(1061)
    centres = 3.0 * rng.standard_normal((8, 33))
    return (centres[rng.randint(0, 8, size=1061)] + rng.standard_normal((1061, 33))).astype(np.float32)


def squared_distances(X):
    X = np.asarray(X, dtype=np.float64)
    D = np.empty((len(X), len(X)))
    for i in range(len(X)):
        D[i] = ((X - X[i]) ** 2).sum(axis=1)
    return D


def knn_bound(X):
    """4 eps32 d max |x - mean|^2."""
    X = np.asarray(X, dtype=np.float64)
    return 4.0 * np.finfo(np.float32).eps * X.shape[1] * ((X - X.mean(axis=0)) ** 2).sum(axis=1).max()


def sorted_knn(D, k):
    """ids (n, k) ascending by (distance, id) without the row itself, and their distances, from the dense fp64 matrix D."""
    D = D.copy()
    np.fill_diagonal(D, np.inf)
    ids = np.lexsort((np.broadcast_to(np.arange(len(D)), D.shape), D), axis=1)[:, :k]
    return ids.astype(np.int32), np.take_along_axis(D, ids, axis=1)


def binary_search_perplexity(dist, perplexity, dtype=np.float64):
    """sklearn/manifold/_utils.pyx _binary_search_perplexity, all rows at once: a row stops changing at the step its entropy is within 1e-5
    of log(perplexity), as the scalar loop's `break` does.  dist (n, k) squared distances, every entry a neighbour."""
    d = np.asarray(dist).astype(dtype)
    n, k = d.shape
    desired = dtype(np.log(perplexity))
    beta = np.ones(n, dtype); lo = np.full(n, -np.inf, dtype); hi = np.full(n, np.inf, dtype)
    P = np.zeros((n, k), dtype)
    live = np.arange(n)
    for _ in range(100):
        b = beta[live]
        Pa = np.exp(-d[live] * b[:, None])
        s = Pa.sum(axis=1, dtype=dtype)
        s[s == 0] = dtype(1e-8)
        Pa = Pa / s[:, None]
        diff = np.log(s) + b * (d[live] * Pa).sum(axis=1, dtype=dtype) - desired
        P[live] = Pa
        go = np.abs(diff) > dtype(1e-5)
        up = go & (diff > 0); down = go & ~(diff > 0)
        r = live[up]
        lo[r] = beta[r]
        beta[r] = np.where(np.isinf(hi[r]), beta[r] * dtype(2), (beta[r] + hi[r]) / dtype(2))
        r = live[down]
        hi[r] = beta[r]
        beta[r] = np.where(np.isinf(lo[r]), beta[r] / dtype(2), (beta[r] + lo[r]) / dtype(2))
        live = live[go]
        if not len(live):
            break
    return P


def dense_joint(n, ids, p, dtype=np.float64):
    """P = (C + C^T) / 2n of the conditional matrix C[i, ids[i, t]] = p[i, t]: sklearn's P + P^T over its sum when every row of C sums to 1."""
    Cm = np.zeros((n, n), dtype)
    np.put_along_axis(Cm, np.asarray(ids, dtype=np.int64), np.asarray(p).astype(dtype), axis=1)
    return (Cm + Cm.T) / dtype(2 * n)


def gradient(P, Y, exaggeration, dtype=np.float64, order=None):
    """(grad (n, 2), KL of the unexaggerated P, Z) of the dense problem: grad_i = 4 sum_j (exaggeration P_ij w_ij - w_ij^2 / Z)(y_i - y_j),
    w = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w, KL = sum_{P > 0} P log(max(P, eps) / max(w / Z, eps)).  order: a permutation of the
    columns the row sums are taken in."""
    P = np.asarray(P).astype(dtype); Y = np.asarray(Y).astype(dtype)
    n = len(Y)
    d0 = Y[:, None, 0] - Y[None, :, 0]; d1 = Y[:, None, 1] - Y[None, :, 1]
    W = dtype(1) / (dtype(1) + d0 * d0 + d1 * d1)
    np.fill_diagonal(W, 0)
    Z = W.sum(dtype=dtype)
    M = dtype(exaggeration) * P * W - W * W / Z
    if order is not None:
        M = M[:, order]; d0 = d0[:, order]; d1 = d1[:, order]
    g = dtype(4) * np.stack([(M * d0).sum(axis=1, dtype=dtype), (M * d1).sum(axis=1, dtype=dtype)], axis=1)
    nz = P > 0
    kl = float((P[nz].astype(np.float64) * np.log(np.maximum(P[nz].astype(np.float64), MACHINE_EPS)
                                                 / np.maximum(W[nz].astype(np.float64) / float(Z), MACHINE_EPS))).sum())
    return g, kl, float(Z)


def gradient_descent(P, Y0, n_iter, exaggeration, momentum, lr, dtype=np.float64, state=None):
    """sklearn/manifold/_t_sne.py _gradient_descent at fixed arguments on gradient() above.  state: (update, gains) to go on from.
    Returns (Y, (update, gains))."""
    Y = np.asarray(Y0).astype(dtype).copy()
    update, gains = (np.zeros_like(Y), np.ones_like(Y)) if state is None else (state[0].copy(), state[1].copy())
    for _ in range(n_iter):
        g = gradient(P, Y, exaggeration, dtype)[0]
        inc = update * g < 0
        gains[inc] += dtype(0.2)
        gains[~inc] *= dtype(0.8)
        np.clip(gains, dtype(0.01), np.inf, out=gains)
        g = g * gains
        update = dtype(momentum) * update - dtype(lr) * g
        Y = Y + update
    return Y, (update, gains)


def dense_p_of_input(X, perplexity=PERPLEXITY):
    """sklearn's _joint_probabilities on the dense problem, fp64: conditional P over all n - 1 other rows, symmetrised, normalised."""
    D = squared_distances(X).astype(np.float32).astype(np.float64)            # sklearn hands float32 distances to the search
    n = len(D)
    off = ~np.eye(n, dtype=bool)
    Cm = np.zeros((n, n))
    Cm[off] = binary_search_perplexity(D[off].reshape(n, n - 1), perplexity).ravel()
    P = Cm + Cm.T
    return P / P.sum()


def dense_kl(P, Y):
    """sklearn's _kl_divergence value: 2 sum_{i < j} P log(max(P, eps) / max(q / sum q, eps))."""
    Y = np.asarray(Y, dtype=np.float64)
    d2 = squared_distances(Y)
    W = 1.0 / (1.0 + d2)
    np.fill_diagonal(W, 0.0)
    Q = np.maximum(W / W.sum(), MACHINE_EPS)
    return float((P * np.log(np.maximum(P, MACHINE_EPS) / Q)).sum())


def trustworthiness(X, Y, n_neighbors):
    """sklearn.manifold.trustworthiness (Euclidean) restated."""
    n = len(X)
    DX = squared_distances(X); DY = squared_distances(Y)
    np.fill_diagonal(DX, np.inf); np.fill_diagonal(DY, np.inf)
    ind_X = np.argsort(DX, axis=1, kind='stable')
    ind_Y = np.argsort(DY, axis=1, kind='stable')[:, :n_neighbors]
    rank = np.empty((n, n), dtype=np.int64)
    np.put_along_axis(rank, ind_X, np.broadcast_to(np.arange(1, n + 1), (n, n)), axis=1)
    r = np.take_along_axis(rank, ind_Y, axis=1) - n_neighbors
    t = r[r > 0].sum()
    return float(1.0 - t * (2.0 / (n * n_neighbors * (2.0 * n - 3.0 * n_neighbors - 1.0))))
