"""Binary ranking metrics on the GPU (gem_amd/csrc/rank.hip): a stable descending device sort of fp64 scores and, on the
sorted sequence, the exact ROC-AUC (twice the Mann-Whitney U as an integer, one division), sklearn's step-wise average precision and the
ROC / precision-recall curve points.  -0.0 ties with +0.0, +-inf are ordinary scores, NaN is refused by position.
No host fallback: GemHipError without a device (binary_scores_from_groups alone is host arithmetic)."""
import ctypes as ct

import numpy as np

from gem_amd import _hip

INFO_FIELDS = ('keys_per_workgroup', 'threads', 'radix_bits', 'passes', 'passes_skipped', 'workgroups', 'n_thresholds', 'm')


def _scores(score):
    s = np.ascontiguousarray(np.asarray(score).ravel(), dtype=np.float64)
    return s


def _labels(label, m):
    y = np.asarray(label).ravel()
    if y.shape[0] != m:
        raise ValueError('label has %d entries, score %d' % (y.shape[0], m))
    if y.dtype == np.bool_:
        return np.ascontiguousarray(y, dtype=np.uint8)
    bad = np.flatnonzero((y != 0) & (y != 1))
    if len(bad):
        raise ValueError('label[%d] = %s is neither 0 nor 1' % (bad[0], y[bad[0]]))
    return np.ascontiguousarray(y, dtype=np.uint8)


def sort_info():
    """gemhip_rank_info of the last sort on this thread, as a dict of INFO_FIELDS."""
    out = (ct.c_int64 * 8)()
    _hip.check(_hip.lib().gemhip_rank_info(out))
    return dict(zip(INFO_FIELDS, (int(v) for v in out)))


def argsort_desc(score):
    """int32 (m,): the positions of the scores in descending order, equal scores in their original order -- numpy.argsort(-score, kind='stable')."""
    s = _scores(score)
    perm = np.zeros(len(s), np.int32)
    _hip.check(_hip.lib().gemhip_rank_argsort(len(s), _hip.ptr(s, ct.c_double), _hip.ptr(perm, ct.c_int32)))
    return perm


def _result(out, counts):
    return {'auc': float(out[0]), 'ap': float(out[1]), 'prevalence': float(out[2]), 'kernel_ms': float(out[3]), 'n_pos': int(counts[0]), 'n_neg': int(counts[1]),
            'n_thresholds': int(counts[2]), 'u2': int(counts[3])}


def binary_ranking_scores(score, label):
    """{'auc', 'ap', 'n_pos', 'n_neg', 'n_thresholds', 'u2', 'prevalence', 'kernel_ms'} of fp64 scores against 0 / 1 labels: sklearn's
    roc_auc_score and average_precision_score, u2 = 2 * P * N * auc exactly."""
    s = _scores(score)
    y = _labels(label, len(s))
    out = (ct.c_double * 4)(); counts = (ct.c_int64 * 4)()
    _hip.check(_hip.lib().gemhip_rank_binary(len(s), _hip.ptr(s, ct.c_double), _hip.ptr(y, ct.c_uint8), out, counts))
    return _result(out, counts)


def binary_scores_from_groups(tp, fp):
    """The same dict (kernel_ms = 0) from the cumulative counts at the end of every tie group, descending score.  Host only."""
    tp = np.ascontiguousarray(tp, dtype=np.int64); fp = np.ascontiguousarray(fp, dtype=np.int64)
    if tp.shape != fp.shape or tp.ndim != 1:
        raise ValueError('tp and fp must be 1-D arrays of equal length')
    out = (ct.c_double * 4)(); counts = (ct.c_int64 * 4)()
    _hip.check(_hip.lib().gemhip_rank_binary_from_groups_host(len(tp), _hip.ptr(tp, ct.c_int64), _hip.ptr(fp, ct.c_int64), out, counts))
    return _result(out, counts)


def group_table(score, label):
    """(thresholds float64, tp int64, fp int64), each (T,): every distinct score, descending, with the cumulative positives and negatives
    ranked at or above it (gemhip_rank_curve)."""
    s = _scores(score)
    y = _labels(label, len(s))
    L = _hip.lib()
    cap = len(s)
    thr = np.zeros(cap); tp = np.zeros(cap, np.int64); fp = np.zeros(cap, np.int64)
    T = ct.c_int64()
    _hip.check(L.gemhip_rank_curve(len(s), _hip.ptr(s, ct.c_double), _hip.ptr(y, ct.c_uint8), cap, _hip.ptr(thr, ct.c_double), _hip.ptr(tp, ct.c_int64),
                                   _hip.ptr(fp, ct.c_int64), ct.byref(T)))
    T = int(T.value)
    return thr[:T].copy(), tp[:T].copy(), fp[:T].copy()


def roc_from_groups(thr, tp, fp):
    """sklearn's roc_curve(drop_intermediate=False) arrays from a group table.  Host arithmetic: one correctly rounded division per point."""
    tp = np.asarray(tp, dtype=np.int64); fp = np.asarray(fp, dtype=np.int64)
    P, N = float(tp[-1]), float(fp[-1])
    return np.concatenate([[0.0], fp / N]), np.concatenate([[0.0], tp / P]), np.concatenate([[np.inf], np.asarray(thr, dtype=np.float64)])


def pr_from_groups(thr, tp, fp):
    """sklearn's precision_recall_curve arrays from a group table.  Host arithmetic."""
    tp = np.asarray(tp, dtype=np.int64); fp = np.asarray(fp, dtype=np.int64)
    precision = tp / (tp + fp).astype(np.float64)
    recall = tp / float(tp[-1])
    return np.concatenate([precision[::-1], [1.0]]), np.concatenate([recall[::-1], [0.0]]), np.asarray(thr, dtype=np.float64)[::-1].copy()


def roc_curve(score, label):
    """(fpr, tpr, thresholds): sklearn.metrics.roc_curve(label, score, drop_intermediate=False), its leading (0, 0, inf) point included."""
    return roc_from_groups(*group_table(score, label))


def precision_recall_curve(score, label):
    """(precision, recall, thresholds) in sklearn.metrics.precision_recall_curve's layout: thresholds ascending, a closing (1, 0) point."""
    return pr_from_groups(*group_table(score, label))
