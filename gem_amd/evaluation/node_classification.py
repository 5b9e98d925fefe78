"""Node classification of an embedding on the GPU (gem_amd/csrc/nc.hip): GEM's fourth evaluation task.

The protocol is the embedding literature's (DeepWalk, node2vec, the GEM survey): split the nodes, fit a one-vs-rest L2 logistic
regression on the training nodes' embedding rows, predict for every test node as many labels as it truly has -- the ones of largest
logit, the lower class id on ties -- and report micro-F1, macro-F1 and subset accuracy.  The fit is the exact minimiser of sklearn's
LogisticRegression(penalty='l2', C, fit_intercept=True) objective (any solver but liblinear) per class, by damped Newton.
No host fallback: GemHipError without a device."""
import ctypes as ct
import math
import warnings

import numpy as np

from gem_amd import _hip
from gem_amd.evaluation._handle import DeviceHandle, embedding_matrix

DEC_TOL = 1e-10                 # a class is converged after the step whose Newton decrement is at most DEC_TOL * max(1, F)
MAX_ITER = 50
INFO_FIELDS = ('iterations', 'backtracks', 'grad_inf', 'decrement', 'converged', 'degenerate')


def label_csr(Y, n):
    """(K, row_ptr int64 (n + 1,), cls int32) of the labels of n nodes.  Y: 1-D integers (one label each, K = max + 1), a dense 0/1
    (n, K) array, or a scipy sparse (n, K) matrix whose stored non-zeros are the labels."""
    if hasattr(Y, 'tocsr'):
        Y = Y.tocsr()
        if Y.shape[0] != n:
            raise ValueError('Y has %d rows, expected %d' % (Y.shape[0], n))
        Y.sum_duplicates()
        Y.eliminate_zeros()
        return int(Y.shape[1]), np.ascontiguousarray(Y.indptr, dtype=np.int64), np.ascontiguousarray(Y.indices, dtype=np.int32)
    Y = np.asarray(Y)
    if Y.ndim == 1:
        if Y.shape[0] != n:
            raise ValueError('Y has %d entries, expected %d' % (Y.shape[0], n))
        if Y.dtype.kind not in 'iu':
            raise ValueError('1-D labels must be integers')
        if n and Y.min() < 0:
            raise ValueError('negative label %d at node %d' % (Y.min(), int(np.argmin(Y))))
        return int(Y.max()) + 1 if n else 0, np.arange(n + 1, dtype=np.int64), np.ascontiguousarray(Y, dtype=np.int32)
    if Y.ndim != 2 or Y.shape[0] != n:
        raise ValueError('Y must be (n,), (n, K) or sparse (n, K)')
    if not np.all((Y == 0) | (Y == 1)):
        bad = np.argwhere((Y != 0) & (Y != 1))[0]
        raise ValueError('Y[%d][%d] is neither 0 nor 1' % (bad[0], bad[1]))
    rows, cols = np.nonzero(Y)
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=row_ptr[1:])
    return int(Y.shape[1]), row_ptr, np.ascontiguousarray(cols, dtype=np.int32)


def split_nodes(n, test_ratio, seed):
    """(train_idx, test_idx) int32: RandomState(seed).permutation(n), the first ceil(test_ratio * n) entries the test rows -- the count
    rule of sklearn's train_test_split.  Upstream's split is unseeded, so no draw of it can be reproduced; this one can."""
    if not 0.0 < test_ratio < 1.0:
        raise ValueError('test_ratio = %r outside (0, 1)' % (test_ratio,))
    n_test = int(math.ceil(test_ratio * n))
    if n_test < 1 or n_test >= n:
        raise ValueError('test_ratio = %r leaves %d test and %d training rows of %d' % (test_ratio, n_test, n - n_test, n))
    perm = np.random.RandomState(seed).permutation(n).astype(np.int32)
    return np.ascontiguousarray(perm[n_test:]), np.ascontiguousarray(perm[:n_test])


def f1_from_counts(tp, fp, fn):
    """(micro-F1, macro-F1) from per-class integer counts: micro = 2 sum TP / (2 sum TP + sum FP + sum FN); macro = the mean over ALL classes
    of 2 TP / (2 TP + FP + FN), a class without a single TP, FP or FN counting 0 (sklearn f1_score's zero_division default)."""
    tp = np.asarray(tp, dtype=np.int64); fp = np.asarray(fp, dtype=np.int64); fn = np.asarray(fn, dtype=np.int64)
    den = 2 * tp + fp + fn
    per_class = np.where(den > 0, 2.0 * tp / np.maximum(den, 1), 0.0)
    total = int(den.sum())
    micro = 2.0 * int(tp.sum()) / total if total else 0.0
    return micro, float(per_class.mean()) if len(per_class) else 0.0


class NodeClassifier(DeviceHandle):
    """gemhip_nc_t with its calls; X is uploaded once: `with NodeClassifier(X) as nc:`."""

    _destroy = 'gemhip_nc_destroy'

    def __init__(self, X, d=None):
        """X (n, ld) float32; d: how many leading columns count (all by default; the rest is padding the device never reads)."""
        DeviceHandle.__init__(self)
        X, self.n, self.d, ld = embedding_matrix(X, d)
        self.K = 0
        _hip.check(_hip.lib().gemhip_nc_create(self.n, self.d, ld, _hip.ptr(X, ct.c_float), ct.byref(self._h)))

    def set_labels(self, Y):
        """Y as label_csr takes it, or a (K, row_ptr, cls) triple."""
        K, row_ptr, cls = Y if isinstance(Y, tuple) else label_csr(Y, self.n)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int64); cls = _hip.as_i32(cls)
        if row_ptr.shape != (self.n + 1,):
            raise ValueError('row_ptr must have n + 1 = %d entries' % (self.n + 1))
        _hip.check(_hip.lib().gemhip_nc_set_labels(self._h, int(K), _hip.ptr(row_ptr, ct.c_int64), _hip.ptr(cls, ct.c_int32)))
        self.K = int(K)

    def _rows(self, idx):
        return np.ascontiguousarray(np.asarray(idx).ravel(), dtype=np.int32)

    def fit(self, train_idx, C=1.0, dec_tol=DEC_TOL, max_iter=MAX_ITER, W0=None, warn=True):
        """-> (coef (K, d), intercept (K,), info).  C=...: sklearn's inverse regularisation strength.  W0: the start, (K, d + 1), zeros by
        default.  info: per class the INFO_FIELDS arrays, plus passes, loss_evaluations, and fit_ms / pass_ms."""
        idx = self._rows(train_idx)
        W = np.zeros((max(self.K, 1), self.d + 1)) if W0 is None else np.array(W0, dtype=np.float64, order='C')
        if self.K and W.shape != (self.K, self.d + 1):
            raise ValueError('W0 must be (%d, %d)' % (self.K, self.d + 1))
        raw = np.zeros((max(self.K, 1), 6))
        _hip.check(_hip.lib().gemhip_nc_fit(self._h, len(idx), _hip.ptr(idx, ct.c_int32), float(C), float(dec_tol), int(max_iter), _hip.ptr(W, ct.c_double),
                                            _hip.ptr(raw, ct.c_double)))
        info = {'iterations': raw[:, 0].astype(np.int64), 'backtracks': raw[:, 1].astype(np.int64), 'grad_inf': raw[:, 2].copy(), 'decrement': raw[:, 3].copy(),
                'converged': raw[:, 4] != 0, 'degenerate': raw[:, 5].astype(np.int64)}
        info.update(self.stats())
        if warn:
            warn_if_unconverged(info, max_iter)
        return W[:, :self.d].copy(), W[:, self.d].copy(), info

    def stats(self):
        ms = (ct.c_double * 4)(); out = (ct.c_int64 * 8)()
        _hip.check(_hip.lib().gemhip_nc_last_ms(self._h, ms))
        _hip.check(_hip.lib().gemhip_nc_info(self._h, out))
        return {'upload_ms': ms[0], 'fit_ms': ms[1], 'pass_ms': ms[2], 'predict_ms': ms[3], 'passes': int(out[3]), 'loss_evaluations': int(out[4]),
                'newton_iterations': int(out[5]), 'class_block': int(out[6]), 'slab_rows': int(out[7])}

    def set_weights(self, coef, intercept=None):
        """coef (K, d) with intercept (K,), or one (K, d + 1) array, w then b."""
        W = np.asarray(coef, dtype=np.float64)
        if intercept is not None:
            W = np.hstack([W, np.asarray(intercept, dtype=np.float64).reshape(-1, 1)])
        W = np.ascontiguousarray(W)
        if self.K and W.shape != (self.K, self.d + 1):
            raise ValueError('weights must be (%d, %d)' % (self.K, self.d + 1))
        _hip.check(_hip.lib().gemhip_nc_set_weights(self._h, _hip.ptr(W, ct.c_double)))

    def pass_(self, train_idx, W, C=1.0):
        """gemhip_nc_pass: (F (K,), g (K, d + 1), H (K, d + 1, d + 1)) of the objective at W (K, d + 1)."""
        idx = self._rows(train_idx)
        W = np.ascontiguousarray(W, dtype=np.float64)
        K, d1 = max(self.K, 1), self.d + 1
        F = np.zeros(K); g = np.zeros((K, d1)); H = np.zeros((K, d1, d1))
        _hip.check(_hip.lib().gemhip_nc_pass(self._h, len(idx), _hip.ptr(idx, ct.c_int32), float(C), _hip.ptr(W, ct.c_double), _hip.ptr(F, ct.c_double),
                                             _hip.ptr(g, ct.c_double), _hip.ptr(H, ct.c_double)))
        return F, g, H

    def decision_function(self, idx):
        """Logits (m, K) float64 of the rows idx."""
        idx = self._rows(idx)
        out = np.zeros((len(idx), max(self.K, 1)))
        _hip.check(_hip.lib().gemhip_nc_scores(self._h, len(idx), _hip.ptr(idx, ct.c_int32), _hip.ptr(out, ct.c_double)))
        return out

    def predict_topk(self, idx, k=None, want_pred=True):
        """-> (pred uint8 (m, K) or None, tp, fp, fn int64 (K,), exact): for row t the k[t] classes of largest logit (its number of true
        labels when k is None), ties to the lower class id; exact = rows whose predicted set is the true set."""
        idx = self._rows(idx)
        K = max(self.K, 1)
        if k is not None:
            k = _hip.as_i32(np.asarray(k).ravel())
            if k.shape != idx.shape:
                raise ValueError('k must have one entry per row')
        pred = np.zeros((len(idx), K), np.uint8) if want_pred else None
        counts = np.zeros((3, K), np.int64)
        exact = ct.c_int64()
        _hip.check(_hip.lib().gemhip_nc_predict_topk(self._h, len(idx), _hip.ptr(idx, ct.c_int32), _hip.ptr(k, ct.c_int32), _hip.ptr(pred, ct.c_uint8),
                                                     _hip.ptr(counts, ct.c_int64), ct.byref(exact)))
        return pred, counts[0], counts[1], counts[2], int(exact.value)


def warn_if_unconverged(info, max_iter):
    bad = np.flatnonzero(~info['converged'])
    if len(bad):
        c = int(bad[0])
        warnings.warn('node classification: %d of %d classes not converged (class %d after %d iterations: decrement %.2e, |g|_inf %.2e); '
                      'raise max_iter (%d) or dec_tol' % (len(bad), len(info['converged']), c, int(info['iterations'][c]), info['decrement'][c],
                                                          info['grad_inf'][c], max_iter), RuntimeWarning, stacklevel=3)


def newton_step_host(H, g):
    """gemhip_nc_newton_step_host (host only, no device): (delta, decrement, shift) with (H + shift I) delta = -g."""
    H = np.ascontiguousarray(H, dtype=np.float64); g = np.ascontiguousarray(g, dtype=np.float64)
    d1 = g.shape[0]
    if H.shape != (d1, d1):
        raise ValueError('H must be (%d, %d)' % (d1, d1))
    delta = np.zeros(d1); dec = ct.c_double(); shift = ct.c_double()
    _hip.check(_hip.lib().gemhip_nc_newton_step_host(d1, _hip.ptr(H, ct.c_double), _hip.ptr(g, ct.c_double), _hip.ptr(delta, ct.c_double), ct.byref(dec),
                                                     ct.byref(shift)))
    return delta, dec.value, shift.value


def _evaluate_on(nc, n, test_ratio, seed, C):
    train, test = split_nodes(n, test_ratio, seed)
    nc.fit(train, C=C)
    _, tp, fp, fn, exact = nc.predict_topk(test, want_pred=False)
    micro, macro = f1_from_counts(tp, fp, fn)
    return micro, macro, exact / float(len(test))


def evaluateNodeClassification(X, Y, test_ratio, seed=0, C=1.0):
    """GEM's name and return order: (micro-F1, macro-F1, accuracy) of one seeded split.  X (n, d) is rounded once to float32."""
    _hip.require_device()
    X = np.asarray(X)
    with NodeClassifier(X) as nc:
        nc.set_labels(Y)
        return _evaluate_on(nc, nc.n, test_ratio, seed, C)


def expNC(X, Y, test_ratio_arr, rounds, seed=0, C=1.0):
    """Every ratio x round on ONE handle (X uploaded once): {ratio: {'micro': [...], 'macro': [...], 'accuracy': [...]}}.  Round r of any ratio
    uses the split of seed + r, so expNC(...)[ratio][...][r] == evaluateNodeClassification(X, Y, ratio, seed + r, C)."""
    _hip.require_device()
    X = np.asarray(X)
    out = {}
    with NodeClassifier(X) as nc:
        nc.set_labels(Y)
        for ratio in test_ratio_arr:
            res = {'micro': [], 'macro': [], 'accuracy': []}
            for r in range(rounds):
                micro, macro, acc = _evaluate_on(nc, nc.n, ratio, seed + r, C)
                res['micro'].append(micro); res['macro'].append(macro); res['accuracy'].append(acc)
            out[ratio] = res
    return out
