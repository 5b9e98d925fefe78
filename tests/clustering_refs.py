"""Host restatements the clustering tests compare gem_amd/csrc/kmeans.hip with (tests/README_clustering.md).  numpy only; `dtype` selects the
precision the distances are carried out in, so the same function is the fp64 reference and the float32 yardstick.  What is restated is
sklearn 1.7.2 KMeans(algorithm='lloyd') on the float32 matrix, with the orders sklearn leaves open fixed as include/gem_hip.h fixes them."""
import os

import numpy as np

import tsne_refs

GOLDEN = tsne_refs.GOLDEN
MFMA_EPS = 1.5e-7                       # the kernel guide's figure for an fp32 MFMA chain of up to 1024 terms, relative to sum |a b|

# name -> (input, K, seed of the start C0 = X[RandomState(seed).choice(n, K, replace=False)])
FIT_SETS = (('prime_k8_s1', 'prime', 8, 1), ('prime_k8_s2', 'prime', 8, 2), ('prime_k13_s0', 'prime', 13, 0), ('prime_k13_s2', 'prime', 13, 2),
            ('normal_k5_s3', 'normal', 5, 3), ('sbm_k3_s1', 'sbm', 3, 1), ('sbm_k3_s3', 'sbm', 3, 3), ('sbm_k7_s1', 'sbm', 7, 1))
RELOCATION_SETS = ('prime_k13_s0', 'prime_k13_s2')
# name -> (input, K, n_local_trials, RandomState seed of the draws)
SEED_SETS = (('prime_k13_t1_s1', 'prime', 13, 1, 1), ('prime_k13_t4_s2', 'prime', 13, 4, 2), ('sbm_k7_t1_s0', 'sbm', 7, 1, 0), ('sbm_k7_t3_s0', 'sbm', 7, 3, 0),
             ('normal_k5_t3_s0', 'normal', 5, 3, 0))


def inputs():
    return {'prime': tsne_refs.prime_input(), 'normal': tsne_refs.normal_input(), 'sbm': tsne_refs.sbm_input().astype(np.float32)}


def sbm_labels():
    return np.load(os.path.join(GOLDEN, 'sbm1024_labels.npy')).astype(np.int32)


def start_centres(X, K, seed):
    return X[np.random.RandomState(seed).choice(len(X), K, replace=False)].copy()


def data_sets():
    """name -> dict(X float32, K, seed, C0, labels_true or None).  Nothing is stored: every input is rebuilt from existing goldens and seeds."""
    X = inputs()
    out = {}
    for name, which, K, seed in FIT_SETS:
        out[name] = {'X': X[which], 'K': K, 'seed': seed, 'C0': start_centres(X[which], K, seed), 'labels_true': sbm_labels() if which == 'sbm' else None}
    return out


def seed_sets():
    X = inputs()
    return {name: {'X': X[which], 'K': K, 'u': np.random.RandomState(seed).uniform(size=(K, T))} for name, which, K, T, seed in SEED_SETS}


# ---------------------------------------------------------------- one step
def assign_ref(X, C, dtype=np.float64):
    """-> (labels int32, score (n, K) in dtype, gap (n,) fp64, B (n,) fp64).  score = |c_k|^2 - 2 x_i . c_k, the arg-min's first occurrence (the
    lower id on ties).  gap: the fp64 second-best minus best score (inf for K = 1).  B_i = 4 * 1.5e-7 * max_k(|c_k|^2 + 2 sum_j |x_ij||c_kj|)."""
    Xd = np.asarray(X).astype(dtype); Cd = np.asarray(C).astype(dtype)
    score = (Cd * Cd).sum(axis=1, dtype=dtype)[None, :] - dtype(2) * (Xd @ Cd.T)
    labels = np.argmin(score, axis=1).astype(np.int32)
    X64 = np.asarray(X, dtype=np.float64); C64 = np.asarray(C, dtype=np.float64)
    s64 = (C64 * C64).sum(axis=1)[None, :] - 2.0 * (X64 @ C64.T)
    part = np.sort(s64, axis=1)
    gap = part[:, 1] - part[:, 0] if s64.shape[1] > 1 else np.full(len(X64), np.inf)
    B = 4.0 * MFMA_EPS * ((C64 * C64).sum(axis=1)[None, :] + 2.0 * (np.abs(X64) @ np.abs(C64).T)).max(axis=1)
    return labels, score, gap, B


def update_ref(X, labels, K, dtype=np.float64):
    """-> (centres float32 (K, d) = float32(sum / count), zeros for an empty cluster; counts int64; sums (K, d) in dtype)."""
    Xd = np.asarray(X).astype(dtype)
    counts = np.bincount(labels, minlength=K).astype(np.int64)
    sums = np.zeros((K, Xd.shape[1]), dtype)
    np.add.at(sums, labels, Xd)
    return centres_of(sums, counts), counts, sums


def centres_of(sums, counts):
    C = np.zeros(sums.shape, np.float32)
    live = counts > 0
    C[live] = (sums[live].astype(np.float64) / counts[live, None]).astype(np.float32)
    return C


def relocate_ref(X, C_old, labels, sums, counts):
    """sklearn's _relocate_empty_clusters_dense with its order fixed: the j-th empty cluster in ascending id takes the row of j-th largest fp64
    squared distance to the old centre of its label, ties to the lower row id; the row leaves its donor.  In place; returns the rows moved."""
    empty = np.flatnonzero(counts == 0)
    if not len(empty):
        return []
    X64 = np.asarray(X, dtype=np.float64)
    dist = ((X64 - np.asarray(C_old, dtype=np.float64)[labels]) ** 2).sum(axis=1)
    far = np.lexsort((np.arange(len(dist)), -dist))[:len(empty)]
    for k, i in zip(empty, far):
        donor = labels[i]
        if counts[donor] <= 1:
            raise ValueError('row %d would leave cluster %d without a row' % (i, donor))
        sums[donor] -= X64[i].astype(sums.dtype)
        sums[k] = X64[i].astype(sums.dtype)
        counts[donor] -= 1
        counts[k] = 1
    return [int(i) for i in far]


def inertia_ref(X, C, labels):
    return float(((np.asarray(X, dtype=np.float64) - np.asarray(C, dtype=np.float64)[labels]) ** 2).sum())


def lloyd(X, C0, tol=1e-4, max_iter=300, dtype=np.float64):
    """sklearn's _kmeans_single_lloyd restated: centres are float32(fp64 sum / count) after every update, distances in `dtype`.
    -> dict(labels, centres, inertia, n_iter, strict, relocated [(iteration, rows)], tight = (row, iteration) pairs with gap <= 2 B,
    pairs = all (row, iteration) pairs)."""
    X = np.asarray(X, dtype=np.float32)
    K = len(C0)
    C = np.asarray(C0, dtype=np.float32).copy()
    tol_abs = tol * float(np.mean(np.var(X.astype(np.float64), axis=0)))
    old = np.full(len(X), -1, np.int32)
    strict = False
    relocated = []
    tight = pairs = 0
    for it in range(max_iter):
        labels, _, gap, B = assign_ref(X, C, dtype)
        tight += int((gap <= 2 * B).sum()); pairs += len(X)
        _, counts, sums = update_ref(X, labels, K)
        rows = relocate_ref(X, C, labels, sums, counts)
        if rows:
            relocated.append((it + 1, rows))
        Cnew = centres_of(sums, counts)
        shift = float(((Cnew.astype(np.float64) - C.astype(np.float64)) ** 2).sum())
        C = Cnew
        n_iter = it + 1
        if np.array_equal(labels, old):
            strict = True
            break
        if shift <= tol_abs:
            break
        old = labels
    if not strict:
        labels = assign_ref(X, C, dtype)[0]
    return {'labels': labels, 'centres': C, 'inertia': inertia_ref(X, C, labels), 'n_iter': n_iter, 'strict': strict, 'relocated': relocated, 'tight': tight,
            'pairs': pairs}


# ---------------------------------------------------------------- seeding
def seed_pp_ref(X, K, u, dtype=np.float64):
    """sklearn's greedy k-means++ on given uniforms u (K, T) -> (rows int32 (K,), margin): centre 0 is row min(floor(u[0][0] n), n - 1); then
    candidates searchsorted(cumsum_fp64(D2), u[c] * total, side='right') clipped to n - 1, D2 the running minimum of difference-form squared
    distances in `dtype`; the smallest fp64 potential wins, ties to the lower trial.  margin: the smallest distance of a draw from a
    cumulative boundary, relative to the total."""
    Xd = np.asarray(X).astype(dtype)
    n = len(Xd)

    def d2(i):
        return ((Xd - Xd[i]) ** 2).sum(axis=1, dtype=dtype)
    rows = [min(int(np.floor(u[0][0] * n)), n - 1)]
    D2 = d2(rows[0])
    margin = np.inf
    for c in range(1, K):
        cs = np.cumsum(D2.astype(np.float64))
        v = u[c] * cs[-1]
        cand = np.minimum(np.searchsorted(cs, v, side='right'), n - 1)
        edges = np.concatenate([[0.0], cs])
        margin = min(margin, float(np.abs(edges[None, :] - v[:, None]).min() / cs[-1]))
        pots = [float(np.minimum(D2, d2(i)).astype(np.float64).sum()) for i in cand]
        best = int(np.argmin(pots))
        rows.append(int(cand[best]))
        D2 = np.minimum(D2, d2(rows[-1]))
    return np.array(rows, np.int32), margin


# ---------------------------------------------------------------- scores
def contingency_ref(pred, true, Kp, Kt):
    return np.bincount(np.asarray(pred, dtype=np.int64) * Kt + np.asarray(true, dtype=np.int64), minlength=Kp * Kt).reshape(Kp, Kt).astype(np.int64)


def scores_ref(table):
    """(nmi, ari, purity) of an integer table in Python integers and fp64: sklearn's definitions restated."""
    t = [[int(v) for v in row] for row in np.asarray(table)]
    a = [sum(row) for row in t]; b = [sum(col) for col in zip(*t)]
    n = sum(a)

    def entropy(m):
        m = [v for v in m if v > 0]
        return 0.0 if len(m) <= 1 else -sum((v / n) * (np.log(v) - np.log(n)) for v in m)
    ra = sum(1 for v in a if v > 0); rb = sum(1 for v in b if v > 0)
    mi = 0.0
    if ra > 1 and rb > 1:
        for i, row in enumerate(t):
            for j, v in enumerate(row):
                if v > 0:
                    mi += (v / n) * (np.log(v) - np.log(n) - np.log(a[i]) - np.log(b[j]) + 2 * np.log(n))
        mi = max(mi, 0.0)
    if ra == 1 and rb == 1:
        nmi = 1.0
    elif mi == 0.0:
        nmi = 0.0
    else:
        nmi = mi / (0.5 * (entropy(a) + entropy(b)))
    ss = sum(v * v for row in t for v in row)
    tp = ss - n; fp = sum(v * v for v in a) - ss; fn = sum(v * v for v in b) - ss; tn = n * n - fp - fn - ss
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    return float(nmi), float(ari), sum(max(row) for row in t) / n
