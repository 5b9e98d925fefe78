"""t-SNE of an embedding to two dimensions on the GPU (gem_amd/csrc/tsne.hip): what upstream's
visualize_embedding.plot_embedding2D does with sklearn.manifold.TSNE(n_components=2) when d > 2 (visualize_embedding.py:9-12).

The schedule is sklearn's (manifold/_t_sne.py): 250 exploration iterations at early exaggeration and momentum 0.5, the rest at
exaggeration 1 and momentum 0.8; every 50 iterations the KL divergence and the gradient norm are read back for the two stop rules.
No host fallback: GemHipError without a device."""
import ctypes as C
import math
import time

import numpy as np

from gem_amd import _hip
from gem_amd.evaluation._handle import DeviceHandle, embedding_matrix

EXPLORATION_ITER = 250                  # sklearn TSNE._EXPLORATION_MAX_ITER
N_ITER_CHECK = 50                       # sklearn TSNE._N_ITER_CHECK
MIN_GRAD_NORM = 1e-7
N_ITER_WITHOUT_PROGRESS = 300
PERPLEXITY_RANGE = (5.0, 100.0)


def pca_init(X):
    """sklearn's init='pca' for two components, on the host in fp64: the two leading eigenvectors of the d x d covariance, each with
    its largest-magnitude entry positive, the scores scaled so that the first column has standard deviation 1e-4.  float32 (n, 2)."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(axis=0)
    d = Xc.shape[1]
    if d == 1:
        Xc = np.hstack([Xc, np.zeros_like(Xc)])
        d = 2
    w, V = np.linalg.eigh(Xc.T @ Xc)
    V = V[:, ::-1][:, :2].copy()
    for c in range(2):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    Y = Xc @ V
    sd = np.std(Y[:, 0])
    if sd > 0:
        Y = Y / sd * 1e-4
    return np.ascontiguousarray(Y, dtype=np.float32)


def learning_rate_auto(n, early_exaggeration):
    """sklearn's learning_rate='auto': max(n / early_exaggeration / 4, 50)."""
    return max(n / early_exaggeration / 4.0, 50.0)


class TsneHandle(DeviceHandle):
    """gemhip_tsne_t with its calls; `with TsneHandle(X, perplexity) as h:`."""

    _destroy = 'gemhip_tsne_destroy'

    def __init__(self, X, perplexity):
        DeviceHandle.__init__(self)
        X, self.n, self.d, _ = embedding_matrix(X)
        _hip.check(_hip.lib().gemhip_tsne_create(self.n, self.d, self.d, _hip.ptr(X, C.c_float), float(perplexity), C.byref(self._h)))
        info = (C.c_int64 * 4)()
        _hip.check(_hip.lib().gemhip_tsne_info(self._h, info))
        self.k, self.n_slices = int(info[2]), int(info[3])

    def set_embedding(self, Y):
        Y = _hip.as_f32(Y)
        if Y.shape != (self.n, 2):
            raise ValueError('Y must be (%d, 2)' % self.n)
        _hip.check(_hip.lib().gemhip_tsne_set_embedding(self._h, _hip.ptr(Y, C.c_float)))

    def get_embedding(self):
        Y = np.empty((self.n, 2), np.float32)
        _hip.check(_hip.lib().gemhip_tsne_get_embedding(self._h, _hip.ptr(Y, C.c_float)))
        return Y

    def set_affinities(self, ids, p):
        ids = _hip.as_i32(ids); p = _hip.as_f32(p)
        if ids.shape != (self.n, self.k) or p.shape != (self.n, self.k):
            raise ValueError('ids and p must be (%d, %d)' % (self.n, self.k))
        _hip.check(_hip.lib().gemhip_tsne_set_affinities(self._h, _hip.ptr(ids, C.c_int32), _hip.ptr(p, C.c_float)))

    def gradient(self, exaggeration=1.0):
        """(grad float32 (n, 2), KL of the unexaggerated P, Z) at the handle's embedding."""
        g = np.empty((self.n, 2), np.float32)
        kl = C.c_double(); z = C.c_double()
        _hip.check(_hip.lib().gemhip_tsne_gradient(self._h, float(exaggeration), _hip.ptr(g, C.c_float), C.byref(kl), C.byref(z)))
        return g, kl.value, z.value

    def run(self, n_iter, exaggeration, momentum, lr):
        """n_iter steps at fixed arguments -> (KL of the unexaggerated P, |gains * grad|) of the last step."""
        kl = C.c_double(); gn = C.c_double()
        _hip.check(_hip.lib().gemhip_tsne_run(self._h, int(n_iter), float(exaggeration), float(momentum), float(lr), C.byref(kl), C.byref(gn)))
        return kl.value, gn.value

    def last_ms(self):
        out = (C.c_double * 4)()
        _hip.check(_hip.lib().gemhip_tsne_last_ms(self._h, out))
        return {'knn_ms': out[0], 'affinity_ms': out[1], 'transpose_ms': out[2], 'run_ms': out[3]}


def knn(X, k):
    """gemhip_tsne_knn: (ids int32 (n, k), squared distances float32 (n, k)), every row ascending by (distance, id)."""
    _hip.require_device()
    X = _hip.as_f32(X)
    n, d = X.shape
    ids = np.empty((n, k), np.int32); dist = np.empty((n, k), np.float32)
    _hip.check(_hip.lib().gemhip_tsne_knn(n, d, d, _hip.ptr(X, C.c_float), int(k), _hip.ptr(ids, C.c_int32), _hip.ptr(dist, C.c_float)))
    return ids, dist


def conditional_affinities(dist, perplexity):
    """gemhip_tsne_affinities: sklearn's _binary_search_perplexity over (n, k) squared distances -> float32 (n, k)."""
    _hip.require_device()
    dist = _hip.as_f32(dist)
    n, k = dist.shape
    p = np.empty((n, k), np.float32)
    _hip.check(_hip.lib().gemhip_tsne_affinities(n, k, _hip.ptr(dist, C.c_float), float(perplexity), _hip.ptr(p, C.c_float)))
    return p


def tsne_2d(X, perplexity=30.0, max_iter=1000, early_exaggeration=12.0, learning_rate='auto', init='pca', verbose=False):
    """(Y float64 (n, 2), info): sklearn.manifold.TSNE(n_components=2, init='pca').fit_transform(X) with the repulsive term summed exactly.
    init: 'pca' or an (n, 2) array.  info: kl_divergence, n_iter, learning_rate, k, and the device time of the phases in milliseconds."""
    _hip.require_device()
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError('X must be (n, d)')
    n = X.shape[0]
    if isinstance(init, str):
        if init != 'pca':
            raise ValueError("init must be 'pca' or an (n, 2) array")
        Y0 = pca_init(X)
    else:
        Y0 = np.ascontiguousarray(init, dtype=np.float32)
        if Y0.shape != (n, 2):
            raise ValueError('init must be (%d, 2)' % n)
    lr = learning_rate_auto(n, early_exaggeration) if learning_rate == 'auto' else float(learning_rate)
    t0 = time.perf_counter()
    with TsneHandle(X, perplexity) as h:
        h.set_embedding(Y0)
        it, kl, run_ms, stopped = 0, float('nan'), 0.0, None
        for phase_end, exaggeration, momentum, patience in ((min(EXPLORATION_ITER, max_iter), early_exaggeration, 0.5, EXPLORATION_ITER),
                                                            (max_iter, 1.0, 0.8, N_ITER_WITHOUT_PROGRESS)):
            best_error, best_iter = float('inf'), it
            while it < phase_end and stopped is None:
                step = min(N_ITER_CHECK - it % N_ITER_CHECK, phase_end - it)
                kl, grad_norm = h.run(step, exaggeration, momentum, lr)
                run_ms += h.last_ms()['run_ms']
                it += step
                if it % N_ITER_CHECK:
                    continue
                error = exaggeration * (kl + math.log(exaggeration))          # KL of the exaggerated P, what sklearn's rule compares
                if verbose:
                    print('[t-SNE] iteration %d: KL = %.6f, gradient norm = %.3e' % (it, kl, grad_norm))
                if error < best_error:
                    best_error, best_iter = error, it - 1
                elif it - 1 - best_iter > patience:
                    stopped = 'no progress'
                if grad_norm <= MIN_GRAD_NORM:
                    stopped = 'gradient norm'
            if stopped is not None and it < EXPLORATION_ITER:
                stopped = None                                                # sklearn goes on to the second phase after an early stop in the first
        Y = h.get_embedding().astype(np.float64)
        ms = h.last_ms()
        k = h.k
    info = {'kl_divergence': kl, 'n_iter': it, 'learning_rate': lr, 'k': k, 'stopped': stopped, 'knn_ms': ms['knn_ms'], 'affinity_ms': ms['affinity_ms'],
            'transpose_ms': ms['transpose_ms'], 'iterations_ms': run_ms, 'wall_s': time.perf_counter() - t0}
    return Y, info
