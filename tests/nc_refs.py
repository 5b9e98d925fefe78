"""Numpy restatements of node classification (tests/README_nc.md): the one-vs-rest logistic objective and its damped Newton fit, the top-k
ranker with the tie rule, the counts -- each with a `dtype` argument, so that the same code is the fp64 reference and the float32 yardstick --
and the data sets the fixtures and tests are built on.  The data sets are rebuilt from existing goldens and seeds, never stored."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ARMIJO_C1 = 1e-4
MAX_HALVINGS = 40


# ------------------------------------------------------------------ objective
def augment(X, dtype=np.float64):
    """x~ = (x, 1) in dtype."""
    X = np.asarray(X, dtype=dtype)
    return np.hstack([X, np.ones((len(X), 1), dtype)])


def sigma_parts(z):
    """(p, 1 - p, log(1 + exp(-|z|))) in z's dtype, in the forms that do not cancel where sigma saturates."""
    e = np.exp(-np.abs(z))
    t = 1 / (1 + e)
    return np.where(z >= 0, t, e * t), np.where(z >= 0, e * t, t), np.log1p(e)


def loss_only(Xa, y01, theta, C):
    z = Xa @ theta
    _, _, l1p = sigma_parts(z)
    terms = l1p + np.where(y01 > 0, np.maximum(-z, 0), np.maximum(z, 0))
    return C * terms.sum() + theta[:-1] @ theta[:-1] / 2


def pass_ref(Xa, y01, theta, C):
    """(F, g, H) of F = C sum log(1 + exp(-y z)) + |w|^2 / 2 at theta = (w, b); everything in Xa's dtype."""
    dt = Xa.dtype
    theta = np.asarray(theta, dtype=dt)
    C = dt.type(C)
    z = Xa @ theta
    p, q, l1p = sigma_parts(z)
    pos = np.asarray(y01) > 0
    F = C * (l1p + np.where(pos, np.maximum(-z, 0), np.maximum(z, 0))).sum() + theta[:-1] @ theta[:-1] / 2
    r = np.where(pos, -q, p)
    s = p * q
    reg = np.ones(len(theta), dt); reg[-1] = 0
    g = C * (Xa.T @ r) + reg * theta
    H = C * ((Xa * s[:, None]).T @ Xa) + np.diag(reg)
    return F, g, H


def newton_fit(X, y01, C=1.0, theta0=None, dtype=np.float64, dec_tol=1e-10, max_iter=50):
    """The solver's iteration restated: Newton step, Armijo backtracking (c1 = 1e-4, halving), a full step without a loss evaluation once
    the decrement is below 450 ulp of max(1, F), converged after the step whose decrement <= dec_tol * max(1, F).
    -> (theta, {'iterations', 'backtracks', 'converged'})."""
    dt = np.dtype(dtype)
    Xa = augment(X, dt)
    theta = np.zeros(Xa.shape[1], dt) if theta0 is None else np.asarray(theta0, dtype=dt).copy()
    full_step = 450 * np.finfo(dt).eps
    info = {'iterations': 0, 'backtracks': 0, 'converged': False}
    for _ in range(max_iter):
        F, g, H = pass_ref(Xa, y01, theta, C)
        delta = np.linalg.solve(H, -g).astype(dt)
        dec = float(-(g @ delta))
        alpha = 1.0
        if dec > full_step * max(1.0, float(F)):
            halvings = 0
            while not loss_only(Xa, y01, theta + dt.type(alpha) * delta, dt.type(C)) <= F - ARMIJO_C1 * alpha * dec:
                if halvings >= MAX_HALVINGS:
                    return theta, info
                alpha *= 0.5
                halvings += 1
                info['backtracks'] += 1
        theta = theta + dt.type(alpha) * delta
        info['iterations'] += 1
        if dec <= dec_tol * max(1.0, float(F)):
            info['converged'] = True
            break
    return theta, info


def fit_all(X, Y01, C=1.0, W0=None, dtype=np.float64, **kw):
    """newton_fit per class of the dense indicator Y01 (n, K) -> (W (K, d + 1), [info])."""
    K = Y01.shape[1]
    out = [newton_fit(X, Y01[:, c], C, None if W0 is None else W0[c], dtype, **kw) for c in range(K)]
    return np.array([o[0] for o in out], dtype=np.float64), [o[1] for o in out]


# ------------------------------------------------------------------ prediction
def topk_ref(scores, k):
    """pred uint8 (m, K): per row the k[i] largest scores, the lower class id on equal scores."""
    scores = np.asarray(scores)
    pred = np.zeros(scores.shape, np.uint8)
    for i in range(len(scores)):
        order = sorted(range(scores.shape[1]), key=lambda c: (-scores[i, c], c))
        pred[i, order[:int(k[i])]] = 1
    return pred


def counts_ref(pred, Ytrue):
    """(tp, fp, fn int64 (K,), exact) of 0/1 arrays (m, K)."""
    pred = np.asarray(pred).astype(bool); Ytrue = np.asarray(Ytrue).astype(bool)
    tp = (pred & Ytrue).sum(0).astype(np.int64); fp = (pred & ~Ytrue).sum(0).astype(np.int64); fn = (~pred & Ytrue).sum(0).astype(np.int64)
    return tp, fp, fn, int((pred == Ytrue).all(1).sum())


def scores_ref(X, W):
    """fp64 logits (m, K) of float32 rows."""
    return augment(np.asarray(X, np.float32), np.float64) @ np.asarray(W, np.float64).T


def min_rank_gap(scores, k):
    """The smallest distance between the k-th and the (k + 1)-th largest sigmoid of a row (rows with 0 < k < K)."""
    p = 1 / (1 + np.exp(-np.asarray(scores, np.float64)))
    gap = np.inf
    for i in range(len(p)):
        ki = int(k[i])
        if 0 < ki < p.shape[1]:
            srt = np.sort(p[i])[::-1]
            gap = min(gap, srt[ki - 1] - srt[ki])
    return gap


# ------------------------------------------------------------------ data sets
SYNTH_SEED, SYNTH_CLASSES, SYNTH_POSITIVE = 5, 5, 0.30
SPLIT_SEED, TEST_RATIO = 0, 0.3
NORMAL_SEED, NORMAL_LABEL_SEED, NORMAL_N, NORMAL_D = 17, 20, 300, 128        # the seeds: scripts/make_golden_nc.py says how they were chosen
LS_SEED, LS_N, LS_D = 26, 1061, 33


def embedding():
    """hope_sbm1024_d32.npz X rounded once to float32, and the reference's block labels."""
    X = np.load(os.path.join(GOLDEN, 'hope_sbm1024_d32.npz'))['X'].astype(np.float32)
    return X, np.load(os.path.join(GOLDEN, 'sbm1024_labels.npy')).astype(np.int64)


def standardised(X):
    X64 = np.asarray(X, np.float64)
    return ((X64 - X64.mean(0)) / X64.std(0)).astype(np.float32)


def multilabel(Xstd, blocks):
    """(n, 8) 0/1: the three blocks plus SYNTH_CLASSES synthetic classes -- seeded linear scores of the standardised columns plus N(0,1)
    noise, the top 30 % positive."""
    rng = np.random.RandomState(SYNTH_SEED)
    n, d = Xstd.shape
    Y = np.zeros((n, 3 + SYNTH_CLASSES), np.uint8)
    Y[np.arange(n), blocks] = 1
    for c in range(SYNTH_CLASSES):
        score = np.asarray(Xstd, np.float64) @ rng.standard_normal(d) + rng.standard_normal(n)
        Y[score >= np.quantile(score, 1 - SYNTH_POSITIVE), 3 + c] = 1
    return Y


def random_labels(n, K, seed, positive=0.30):
    return (np.random.RandomState(seed).random_sample((n, K)) < positive).astype(np.uint8)


def data_sets():
    """name -> dict(X float32, Y uint8 (n, K), C, W0 or None, predict: is it a prediction set).  Training rows: split(n) below."""
    X, blocks = embedding()
    Xstd = standardised(X)
    Y8 = multilabel(Xstd, blocks)
    Xn = np.random.RandomState(NORMAL_SEED).standard_normal((NORMAL_N, NORMAL_D)).astype(np.float32)
    Yn = random_labels(NORMAL_N, 2, NORMAL_LABEL_SEED)
    rng = np.random.RandomState(LS_SEED)
    Xl = (3 * rng.standard_normal((LS_N, LS_D))).astype(np.float32)
    Yl = random_labels(LS_N, 2, LS_SEED + 1)
    W0l = 5 * rng.standard_normal((2, LS_D + 1))
    return {
        'std': dict(X=Xstd, Y=Y8, C=1.0, W0=None, predict=True),
        'x100': dict(X=(100 * X).astype(np.float32), Y=Y8, C=1.0, W0=None, predict=True),
        'raw': dict(X=X, Y=Y8[:, :3], C=1.0, W0=None, predict=False),
        'normal': dict(X=Xn, Y=Yn, C=1.0, W0=None, predict=False),
        'normal_C1e4': dict(X=Xn, Y=Yn, C=1e4, W0=None, predict=False),
        'warm': dict(X=Xl, Y=Yl, C=1.0, W0=W0l, predict=False),
    }


LINE_SEARCH_SETS = ('normal_C1e4', 'warm')


def train_rows(name, n):
    """The training rows of a data set: the split's on the prediction sets, otherwise every row once, shuffled (seed 1)."""
    if name in ('std', 'x100'):
        return split(n)[0]
    return np.random.RandomState(1).permutation(n).astype(np.int32)


def split(n):
    """(train, test) as gem_amd.evaluation.node_classification.split_nodes(n, TEST_RATIO, SPLIT_SEED) makes them."""
    n_test = int(np.ceil(TEST_RATIO * n))
    perm = np.random.RandomState(SPLIT_SEED).permutation(n).astype(np.int32)
    return perm[n_test:], perm[:n_test]
