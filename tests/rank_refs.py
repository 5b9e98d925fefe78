"""Restatements for the ranking metrics and link classification (tests/README_link_auc.md): the stable descending argsort, the group table
and ROC-AUC / average precision as exact rationals in Python integers, the four pair operators in numpy float32, sklearn's curve layouts from
a group table -- and the data sets the fixture and the tests are built on, rebuilt from existing goldens and seeds, never stored."""
import os
from fractions import Fraction

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
OPS = ('average', 'hadamard', 'l1', 'l2')
SPLIT_SEED, PAIR_SEED, TRAIN_SHARE = 3, 0, 0.5
CURVE_SEED, CURVE_M, CURVE_STEP = 11, 3000, 64


# ------------------------------------------------------------------ sort and metrics
def argsort_ref(s):
    """numpy's stable sort of -s: descending, equal scores (and the two zeros) in their original order."""
    return np.argsort(-np.asarray(s, dtype=np.float64), kind='stable').astype(np.int32)


def exact_scores(s, y):
    """The group table and the metrics in exact arithmetic.  -> dict: thr (list of float), tp, fp (lists of int, cumulative at each distinct
    score, descending), P, N, T, U2 (int), auc, ap (Fraction)."""
    s = np.asarray(s, dtype=np.float64); y = np.asarray(y).astype(np.int64)
    order = argsort_ref(s)
    ss, yy = s[order], y[order]
    ends = np.flatnonzero(np.append(ss[1:] != ss[:-1], True))            # 0.0 == -0.0: one group
    tp = np.cumsum(yy)[ends].tolist()
    fp = (ends + 1 - np.cumsum(yy)[ends]).tolist()
    P, N, T = int(tp[-1]), int(fp[-1]), len(ends)
    U2, ap, ptp, pfp = 0, Fraction(0), 0, 0
    for g in range(T):
        pos, neg = tp[g] - ptp, fp[g] - pfp
        U2 += pos * (2 * (N - fp[g]) + neg)
        ap += Fraction(pos * tp[g], tp[g] + fp[g])
        ptp, pfp = tp[g], fp[g]
    return {'thr': ss[ends].tolist(), 'tp': tp, 'fp': fp, 'P': P, 'N': N, 'T': T, 'U2': U2,
            'auc': Fraction(U2, 2 * P * N) if P and N else None, 'ap': ap / P if P else None}


def roc_ref(ex):
    """sklearn.metrics.roc_curve(drop_intermediate=False) from a group table, as exact rationals: (fpr, tpr) lists of Fraction."""
    return [Fraction(0)] + [Fraction(f, ex['N']) for f in ex['fp']], [Fraction(0)] + [Fraction(t, ex['P']) for t in ex['tp']]


def pr_ref(ex):
    """sklearn.metrics.precision_recall_curve from a group table, as exact rationals: (precision, recall), thresholds ascending, closing (1, 0)."""
    prec = [Fraction(t, t + f) for t, f in zip(ex['tp'], ex['fp'])][::-1] + [Fraction(1)]
    rec = [Fraction(t, ex['P']) for t in ex['tp']][::-1] + [Fraction(0)]
    return prec, rec


def max_dev(values, fractions):
    """The largest |float - Fraction| of two equally long sequences, as a float."""
    return float(max([abs(Fraction(float(v)) - f) for v, f in zip(values, fractions)] + [Fraction(0)]))


# ------------------------------------------------------------------ pair operators
def op_ref(op, A, B):
    """The operator on float32 rows, every step rounded to float32."""
    A = np.asarray(A, dtype=np.float32); B = np.asarray(B, dtype=np.float32)
    if op in ('average', 0):
        return (A + B) * np.float32(0.5)
    if op in ('hadamard', 1):
        return A * B
    t = A - B
    if op in ('l1', 2):
        return np.abs(t)
    if op in ('l2', 3):
        return t * t
    raise ValueError(op)


def features_ref(op, X, st, ed):
    X = np.asarray(X, dtype=np.float32)
    return op_ref(op, X[np.asarray(st)], X[np.asarray(ed)])


def scores_ref(F, w):
    """fp64 logits of float32 features."""
    w = np.asarray(w, dtype=np.float64)
    return np.asarray(F, np.float32).astype(np.float64) @ w[:-1] + w[-1]


def score_bound(F, w):
    """4 (d + 1) 2^-53 (sum_j |f_j w_j| + |b|): what any order of fp64 products and sums stays inside."""
    w = np.asarray(w, dtype=np.float64)
    F = np.asarray(F, np.float32).astype(np.float64)
    return 4 * (F.shape[1] + 1) * 2.0 ** -53 * (np.abs(F) @ np.abs(w[:-1]) + abs(w[-1]))


# ------------------------------------------------------------------ sensitivities of the end-to-end figures
def near_pairs(s, y, delta):
    """How many (positive, negative) pairs have scores within delta of each other: the pairs a perturbation of the scores can reorder."""
    s = np.asarray(s, dtype=np.float64); y = np.asarray(y).astype(bool)
    neg = np.sort(s[~y])
    return int((np.searchsorted(neg, s[y] + delta, side='right') - np.searchsorted(neg, s[y] - delta, side='left')).sum())


def ap_sensitivity(s, y, delta):
    """A bound on |AP(s') - AP(s)| for any s' whose pairwise differences are within delta of s's.  For a positive i, tp_i (positives ranked
    at or above it) lies between the count of s > s_i + delta plus itself and the count of s >= s_i - delta, fp_i likewise; its precision
    then lies in [tp_lo / (tp_lo + fp_hi), tp_hi / (tp_hi + fp_lo)], and AP is the mean of the positives' precisions."""
    s = np.asarray(s, dtype=np.float64); y = np.asarray(y).astype(bool)
    pos, neg = np.sort(s[y]), np.sort(s[~y])
    si = s[y]
    tp = len(pos) - np.searchsorted(pos, si, side='left'); fp = len(neg) - np.searchsorted(neg, si, side='left')
    tp_lo = len(pos) - np.searchsorted(pos, si + delta, side='right') + 1; tp_hi = len(pos) - np.searchsorted(pos, si - delta, side='left')
    fp_lo = len(neg) - np.searchsorted(neg, si + delta, side='right'); fp_hi = len(neg) - np.searchsorted(neg, si - delta, side='left')
    p = tp / (tp + fp).astype(np.float64)
    lo = tp_lo / (tp_lo + fp_hi).astype(np.float64); hi = tp_hi / (tp_hi + fp_lo).astype(np.float64)
    return float(np.maximum(hi - p, p - lo).mean())


# ------------------------------------------------------------------ data sets
def embedding():
    """hope_sbm1024_d32.npz X rounded once to float32."""
    return np.load(os.path.join(GOLDEN, 'hope_sbm1024_d32.npz'))['X'].astype(np.float32)


def split_graphs():
    """(train, test) EdgeListGraphs of the SBM-1024 golden graph: every undirected edge goes to the train graph with probability TRAIN_SHARE on
    RandomState(SPLIT_SEED), in ascending (u, v) order, both orientations together."""
    from gem_amd.graph import EdgeListGraph
    e = np.load(os.path.join(GOLDEN, 'sbm1024_edges.npy')).astype(np.int64)
    n = 1024
    key = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))
    u, v = key // n, key % n
    to_train = np.random.RandomState(SPLIT_SEED).random_sample(len(key)) < TRAIN_SHARE

    def both(mask):
        return EdgeListGraph(n, np.concatenate([u[mask], v[mask]]), np.concatenate([v[mask], u[mask]]))
    return both(to_train), both(~to_train)


def fixture_pairs():
    """gem_amd.evaluation.link_classification.link_pairs on the split above with PAIR_SEED: host code."""
    from gem_amd.evaluation import link_classification as LC
    train, test = split_graphs()
    return train, test, LC.link_pairs(train, test, seed=PAIR_SEED, is_undirected=True)


def curve_set():
    """(score, label): CURVE_M scores quantised to 1 / CURVE_STEP, heavy ties, labels correlated with the score."""
    rng = np.random.RandomState(CURVE_SEED)
    y = (rng.random_sample(CURVE_M) < 0.4).astype(np.uint8)
    s = np.round((rng.standard_normal(CURVE_M) + 0.8 * y) * CURVE_STEP) / CURVE_STEP
    return s, y


def metric_sets():
    """name -> (score float64, label uint8): the sets the metrics are checked on."""
    rng = np.random.RandomState(5)
    big = 1 << 17
    out = {}
    y = (rng.random_sample(4099) < 0.3).astype(np.uint8)
    cont = rng.standard_normal(4099) + y
    out['continuous'] = (cont, y)
    out['quantised_8'] = (np.round(cont * 8) / 8, y)
    out['quantised_64'] = (np.round(cont * 64) / 64, y)
    out['separated_up'] = (np.where(y > 0, 2.0, -1.0) + 0.25 * rng.random_sample(4099), y)
    out['separated_down'] = (-out['separated_up'][0], y)
    out['all_tied'] = (np.full(4099, 0.75), y)
    one = np.zeros(big + 1, np.uint8); one[0] = 1
    out['one_positive_first'] = (-np.arange(big + 1, dtype=np.float64), one)
    out['one_positive_last'] = (np.arange(big + 1, dtype=np.float64), one)
    return out
