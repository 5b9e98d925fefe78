"""Clustering an embedding on the GPU and scoring the clusters against planted communities (gem_amd/csrc/kmeans.hip).

k-means is sklearn 1.7.2's KMeans(algorithm='lloyd') on the float32 matrix, restated exactly where sklearn leaves an order open (ties to
the lower cluster id, the relocation order of empty clusters, the k-means++ draws supplied by the host); the scores are sklearn.metrics'
normalized_mutual_info_score and adjusted_rand_score, plus purity, from an integer contingency table.  Laplacian Eigenmaps followed by
evaluateClustering(normalize='l2') is spectral clustering (Ng, Jordan, Weiss).  No host fallback: GemHipError without a device -- only
clustering_scores works without one."""
import ctypes as ct
import math
import warnings

import numpy as np

from gem_amd import _hip
from gem_amd.evaluation._handle import DeviceHandle, embedding_matrix

TOL = 1e-4
MAX_ITER = 300
INFO_FIELDS = ('n', 'd', 'd_padded', 'K', 'assign_rows', 'centre_tile', 'max_d', 'max_K', 'max_trials', 'slice_members', 'slab_rows', 'iterations')


def default_trials(K):
    """sklearn's n_local_trials: 2 + int(log K)."""
    return 2 + int(math.log(K))


def seed_uniforms(K, seed, n_local_trials=None):
    """The draws seed_pp hands to the device: RandomState(seed).uniform(size=(K, n_local_trials)); row c belongs to centre c, centre 0 uses
    u[0][0] only."""
    T = default_trials(K) if n_local_trials is None else int(n_local_trials)
    return np.random.RandomState(seed).uniform(size=(int(K), T))


def clustering_scores(table):
    """(nmi, ari, purity, homogeneity) of an integer contingency table (rows: predicted clusters, columns: true classes).  Host only."""
    table = np.ascontiguousarray(table, dtype=np.int64)
    if table.ndim != 2:
        raise ValueError('table must be (K_pred, K_true)')
    out = (ct.c_double * 4)()
    _hip.check(_hip.lib().gemhip_clustering_scores_host(_hip.ptr(table, ct.c_int64), table.shape[0], table.shape[1], out))
    return out[0], out[1], out[2], out[3]


def l2_normalize(X):
    """Rows scaled to unit Euclidean norm in float32; zero rows stay zero."""
    X = np.asarray(X, dtype=np.float32)
    norm = np.sqrt((X.astype(np.float64) ** 2).sum(axis=1))
    return (X / np.where(norm > 0, norm, 1.0)[:, None]).astype(np.float32)


class KMeans(DeviceHandle):
    """gemhip_kmeans_t with its calls; X is uploaded once: `with KMeans(X) as km:`."""

    _destroy = 'gemhip_kmeans_destroy'

    def __init__(self, X, d=None):
        """X (n, ld) float32; d: how many leading columns count (all by default; the rest is padding the device never reads)."""
        DeviceHandle.__init__(self)
        X, self.n, self.d, ld = embedding_matrix(X, d)
        _hip.check(_hip.lib().gemhip_kmeans_create(self.n, self.d, ld, _hip.ptr(X, ct.c_float), ct.byref(self._h)))

    def _centres(self, K, centres):
        C = np.array(centres, dtype=np.float32, order='C')
        if C.shape != (int(K), self.d):
            raise ValueError('centres must be (%d, %d)' % (K, self.d))
        return C

    def seed_pp(self, K, seed=0, n_local_trials=None, u=None):
        """-> (rows int32 (K,), centres float32 (K, d)): greedy k-means++ on the draws seed_uniforms(K, seed, n_local_trials), or on u."""
        u = seed_uniforms(K, seed, n_local_trials) if u is None else np.ascontiguousarray(u, dtype=np.float64)
        if u.ndim != 2 or u.shape[0] != int(K):
            raise ValueError('u must be (K, n_local_trials)')
        rows = np.zeros(max(int(K), 1), np.int32); C = np.zeros((max(int(K), 1), self.d), np.float32)
        _hip.check(_hip.lib().gemhip_kmeans_seed_pp(self._h, int(K), u.shape[1], _hip.ptr(u, ct.c_double), _hip.ptr(rows, ct.c_int32), _hip.ptr(C, ct.c_float)))
        return rows, C

    def _fit_once(self, K, C, tol, max_iter):
        labels = np.zeros(self.n, np.int32)
        raw = np.zeros(6)
        _hip.check(_hip.lib().gemhip_kmeans_fit(self._h, int(K), _hip.ptr(C, ct.c_float), float(tol), int(max_iter), _hip.ptr(labels, ct.c_int32),
                                                _hip.ptr(raw, ct.c_double)))
        info = {'inertia': raw[0], 'iterations': int(raw[1]), 'strict': raw[2] != 0, 'relocations': int(raw[3]), 'shift': raw[4], 'tol_abs': raw[5]}
        info['converged'] = info['strict'] or info['shift'] <= info['tol_abs']
        return labels, C, info

    def fit(self, K, init='k-means++', seed=0, n_init=1, tol=TOL, max_iter=MAX_ITER, warn=True):
        """-> (labels int32 (n,), centres float32 (K, d), info).  init: 'k-means++' (run r seeds with RandomState(seed + r)) or a (K, d) array
        (n_init runs of it would be the same run: only one is made).  With n_init > 1 the run of lowest inertia is kept, the earlier on
        ties.  info: inertia, iterations, strict, relocations, shift, tol_abs, converged, run, plus stats()."""
        if n_init < 1:
            raise ValueError('n_init = %r (need >= 1)' % (n_init,))
        given = not isinstance(init, str)
        if not given and init != 'k-means++':
            raise ValueError("init must be 'k-means++' or a (K, d) array")
        best = None
        for r in range(1 if given else int(n_init)):
            C = self._centres(K, init) if given else self.seed_pp(K, seed + r)[1]
            labels, C, info = self._fit_once(K, C, tol, max_iter)
            info['run'] = r
            if best is None or info['inertia'] < best[2]['inertia']:
                best = (labels, C, info)
        labels, C, info = best
        if not given and info['run'] != int(n_init) - 1:
            self.assign(K, C)                                    # the device's labels are the kept run's again (contingency reads them)
        info.update(self.stats())
        if warn:
            warn_if_unconverged(info, max_iter)
        return labels, C, info

    def assign(self, K, centres, want_score=False):
        """One assign step: labels int32 (n,), with want_score also the fp32 score |c|^2 - 2 x . c of the chosen centre."""
        C = self._centres(K, centres)
        labels = np.zeros(self.n, np.int32)
        score = np.zeros(self.n, np.float32) if want_score else None
        _hip.check(_hip.lib().gemhip_kmeans_assign(self._h, int(K), _hip.ptr(C, ct.c_float), _hip.ptr(labels, ct.c_int32), _hip.ptr(score, ct.c_float)))
        return (labels, score) if want_score else labels

    def update(self, K, labels):
        """One update step without relocation: (centres float32 (K, d), zeros for an empty cluster; counts int64 (K,))."""
        labels = _hip.as_i32(np.asarray(labels).ravel())
        if labels.shape != (self.n,):
            raise ValueError('labels must have n = %d entries' % self.n)
        C = np.zeros((max(int(K), 1), self.d), np.float32); counts = np.zeros(max(int(K), 1), np.int64)
        _hip.check(_hip.lib().gemhip_kmeans_update(self._h, int(K), _hip.ptr(labels, ct.c_int32), _hip.ptr(C, ct.c_float), _hip.ptr(counts, ct.c_int64)))
        return C, counts

    def contingency(self, labels_true, n_classes=None):
        """table int64 (K, n_classes) of the device's labels (the last fit, assign or update) against labels_true."""
        lt = np.asarray(labels_true).ravel()
        if lt.shape != (self.n,):
            raise ValueError('labels_true must have n = %d entries' % self.n)
        if lt.dtype.kind not in 'iu':
            raise ValueError('labels_true must be integers')
        lt = _hip.as_i32(lt)
        Kt = int(lt.max()) + 1 if n_classes is None else int(n_classes)
        K = self.stats()['K']
        table = np.zeros((max(K, 1), max(Kt, 1)), np.int64)
        _hip.check(_hip.lib().gemhip_kmeans_contingency(self._h, Kt, _hip.ptr(lt, ct.c_int32), _hip.ptr(table, ct.c_int64)))
        return table

    def stats(self):
        ms = (ct.c_double * 6)(); out = (ct.c_int64 * 12)()
        _hip.check(_hip.lib().gemhip_kmeans_last_ms(self._h, ms))
        _hip.check(_hip.lib().gemhip_kmeans_info(self._h, out))
        s = {'upload_ms': ms[0], 'seed_ms': ms[1], 'fit_ms': ms[2], 'iteration_ms': ms[3], 'assign_ms': ms[4], 'update_ms': ms[5]}
        s.update((name, int(out[q])) for q, name in enumerate(INFO_FIELDS) if name != 'iterations')
        return s


def warn_if_unconverged(info, max_iter):
    if not info['converged']:
        warnings.warn('k-means: not converged after max_iter = %d iterations (centre shift %.3e above tol %.3e); raise max_iter or tol'
                      % (max_iter, info['shift'], info['tol_abs']), RuntimeWarning, stacklevel=3)


def _evaluate_on(km, labels_true, n_clusters, n_classes, init, seed, n_init, tol, max_iter):
    labels, _, info = km.fit(n_clusters, init=init, seed=seed, n_init=n_init, tol=tol, max_iter=max_iter)
    nmi, ari, purity, _ = clustering_scores(km.contingency(labels_true, n_classes))
    return nmi, ari, purity, info['inertia'], labels


def _prepare(X, labels_true, n_clusters, normalize):
    labels_true = np.asarray(labels_true).ravel()
    if labels_true.dtype.kind not in 'iu':
        raise ValueError('labels_true must be integers')
    if normalize not in (None, 'l2'):
        raise ValueError("normalize must be None or 'l2'")
    X = np.asarray(X, dtype=np.float32)
    if normalize == 'l2':
        X = l2_normalize(X)
    K = len(np.unique(labels_true)) if n_clusters is None else int(n_clusters)
    return X, labels_true, K


def evaluateClustering(X, labels_true, n_clusters=None, seed=0, n_init=1, normalize=None, init='k-means++', tol=TOL, max_iter=MAX_ITER,
                       return_labels=False):
    """(nmi, ari, purity, inertia) of k-means++ / Lloyd clusters of the rows of X against labels_true (integers >= 0).  n_clusters: the number
    of distinct true labels by default.  normalize='l2': rows scaled to unit norm first (zero rows stay zero).  init: as KMeans.fit takes it.
    X (n, d) is rounded once to float32."""
    _hip.require_device()
    X, labels_true, K = _prepare(X, labels_true, n_clusters, normalize)
    with KMeans(X) as km:
        nmi, ari, purity, inertia, labels = _evaluate_on(km, labels_true, K, None, init, seed, n_init, tol, max_iter)
    return (nmi, ari, purity, inertia, labels) if return_labels else (nmi, ari, purity, inertia)


def expClustering(X, labels_true, rounds, seed=0, n_clusters=None, n_init=1, normalize=None, init='k-means++', tol=TOL, max_iter=MAX_ITER):
    """Every round on ONE handle (X uploaded once): {'nmi': [...], 'ari': [...], 'purity': [...], 'inertia': [...], 'mean': {...}}.  Round r
    uses seed + r, so the r-th entries equal evaluateClustering(X, labels_true, seed=seed + r, ...)."""
    _hip.require_device()
    X, labels_true, K = _prepare(X, labels_true, n_clusters, normalize)
    res = {'nmi': [], 'ari': [], 'purity': [], 'inertia': []}
    with KMeans(X) as km:
        for r in range(rounds):
            nmi, ari, purity, inertia, _ = _evaluate_on(km, labels_true, K, None, init, seed + r, n_init, tol, max_iter)
            res['nmi'].append(nmi); res['ari'].append(ari); res['purity'].append(purity); res['inertia'].append(inertia)
    res['mean'] = {k: float(np.mean(res[k])) for k in ('nmi', 'ari', 'purity', 'inertia')}
    return res
