"""Device-free references, inputs and DERIVED bounds for the three reporting instruments:

  eval_ap_kernel<NV, KIND, MASKED>  (gem_amd/csrc/eval.hip)  sampled AP        -> test_eval_ap_gpu.py, test_link_prediction_gpu.py;
                             its host half (gem_amd/csrc/eval_host.hip) on the CPU  -> test_eval_host.py
  gf_objective_kernel        (gem_amd/csrc/gf.hip)     f1, f2 of gf.cpp:94-113  -> test_gf_objective_gpu.py
  svd_error_impl             (gem_amd/csrc/hope.hip)   `SVD error (low rank)`   -> test_hope_svd_error_gpu.py

Everything here is numpy in fp64 (or a numpy emulation of a kernel's own arithmetic) and runs without a device; test_instrument_refs.py
holds every bound against that emulation, and shows that a planted mistake breaks it, on the very shapes the GPU tests use."""
import numpy as np

from gem_amd.graph import to_csr

# ====================================================================================================================== sampled AP
AP_N = 700
AP_HUB, AP_512, AP_513, AP_EMPTY, AP_LOWER, AP_TWICE, AP_FAR = 2, 5, 9, 11, 650, 20, 333
# (da, pad, kind, split): every eval_ap_kernel<NV, KIND, false> instantiation, the `cc < da` tail on either side of every NV boundary, ld > da
# (ld = da + 3 at two widths, ld = da + 1 at an even one), the two HOPE splits (A != B), and the distance kernel
AP_CASES = [(da, {63: 3, 257: 3, 128: 1}.get(da, 0), 0, False) for da in (1, 63, 64, 65, 128, 129, 182, 256, 257, 509, 512)] + \
           [(91, 0, 0, True), (200, 0, 0, True)] + [(da, 0, 1, False) for da in (63, 65, 182, 257, 512)]
AP_GRID_BAR = 1e-12            # half-integer inputs: every score is exact, AP is a ratio of small integers summed in fp64
AP_RANDOM_BAR = 1e-9           # the project's per-node bar (test_eval_gpu.py)


def ap_seed(da, kind):
    """The seed of a case's operands; test_instrument_refs.py checks on the CPU that the random family is clear of ties at it."""
    return da + 7 * kind


def ap_graph():
    """One directed graph on 700 nodes: node 2 has 600 neighbours (two chunks of the kernel), node 5 exactly 512, node 9 exactly 513 (all of
    them above the node's id, so the counts hold with and without `undirected`), row 11 is empty, node 650 has lower ids only (no candidate
    when undirected), row 20 is unsorted and lists column 400 twice.  Returns (row_ptr, col, truth)."""
    n = AP_N
    rng = np.random.RandomState(31)
    special = (AP_HUB, AP_512, AP_513, AP_EMPTY, AP_LOWER, AP_TWICE)
    src = rng.randint(0, n, 3000); dst = rng.randint(0, n, 3000)
    keep = ~np.isin(src, special)
    src, dst = [src[keep]], [dst[keep]]
    for node, deg in ((AP_HUB, 600), (AP_512, 512), (AP_513, 513)):
        src.append(np.full(deg, node)); dst.append(rng.choice(np.arange(node + 1, n), deg, replace=False))
    src.append(np.full(3, AP_LOWER)); dst.append(np.array([4, 17, 649]))
    key = np.unique(np.concatenate(src).astype(np.int64) * n + np.concatenate(dst))
    src = np.concatenate([key // n, np.full(5, AP_TWICE)]); dst = np.concatenate([key % n, [400, 17, 400, 333, 21]])
    row_ptr, col, _ = to_csr(n, src, dst, None)                      # stable: row 20 keeps the order above
    assert row_ptr[AP_EMPTY + 1] == row_ptr[AP_EMPTY] and row_ptr[AP_512 + 1] - row_ptr[AP_512] == 512
    assert list(col[row_ptr[AP_TWICE]:row_ptr[AP_TWICE + 1]]) == [400, 17, 400, 333, 21]
    truth = np.zeros((n, n), dtype=bool); truth[src, dst] = True
    return row_ptr, col, truth


def _padded(vals, pad):
    n, da = vals.shape
    out = np.full((n, da + pad), np.float32(1e30)); out[:, :da] = vals          # a read of A or B past da would swamp every score
    return out


def ap_operands(da, pad, kind, split, family, seed):
    """A, B ([n][da + pad] float32, B None unless split) of one case.  family 'grid': multiples of 1/2 in [-2, 2], so that every product and
    every partial sum is exact in fp64 in any order (|sum| < 2^11 in multiples of 1/4) and exact ties are plentiful; kind 1: every row is one
    base row changed in four coordinates by +-1/2 or +-1 (squared distances between 0 and 16), row 333 is moved 16 away in eight coordinates
    (squared distance >= 1800: exp underflows to 0).  family 'random': fp32 normals, scaled by 0.7 / sqrt(da) for kind 1."""
    n = AP_N
    rng = np.random.RandomState(seed)

    def grid(shape):
        return np.clip(np.round(rng.randn(*shape) * 2) / 2, -2, 2)
    if family == 'grid' and kind == 1:
        X = np.repeat(grid((1, da)), n, axis=0)
        for i in range(n):
            c = rng.choice(da, min(4, da), replace=False)
            X[i, c] += rng.choice([-1.0, -0.5, 0.5, 1.0], len(c))
        X[AP_FAR, :min(8, da)] += 16.0
        return _padded(X.astype(np.float32), pad), None
    if family == 'grid':
        return _padded(grid((n, da)).astype(np.float32), pad), (_padded(grid((n, da)).astype(np.float32), pad) if split else None)
    scale = 1.0 if kind == 0 else 0.7 / np.sqrt(da)
    A = _padded((rng.randn(n, da) * scale).astype(np.float32), pad)
    return A, (_padded(rng.randn(n, da).astype(np.float32), pad) if split else None)


def ap_dense_scores(A, B, da, kind):
    """The dense fp64 score matrix of the fp32 inputs, as get_reconstructed_adj forms it, and the magnitude each score's rounding scales with:
    sum_k |a_k b_k| (kind 0) or s (D + 1) for s = exp(-D) (kind 1)."""
    a = A[:, :da].astype(np.float64); b = a if B is None else B[:, :da].astype(np.float64)
    if kind == 0:
        return a @ b.T, np.abs(a) @ np.abs(b).T
    n = a.shape[0]
    s = np.empty((n, n)); D = np.empty((n, n))
    for r in range(0, n, 50):
        diff = a[r:r + 50, None, :] - a[None, :, :]
        D[r:r + 50] = (diff * diff).sum(axis=2)
        s[r:r + 50] = np.exp(-np.linalg.norm(diff, axis=2) ** 2)                 # lap.py:74
    np.fill_diagonal(s, 0.0)
    return s, s * (D + 1.0)


def ap_reference_is_clear_of_ties(score, mag, da):
    """A condition on the INPUT of the random family, not a tolerance: the kernel sums the same fp64 products in another order, which moves a
    score by at most (da - 1) 2^-53 sum|a_k b_k| on either side.  If two distinct candidate scores of one node (or a score and the `> 0`
    filter's zero) are closer than 8 da 2^-53 times that magnitude, the fp64 reference itself does not decide their order."""
    n = score.shape[0]
    for i in range(n):
        keep = np.arange(n) != i
        s = np.sort(np.concatenate([score[i, keep], [0.0]]))
        gap = np.diff(s)
        gap = gap[gap > 0]
        if gap.size and gap.min() <= 8 * da * 2.0 ** -53 * mag[i, keep].max():
            return False
    return True


def ap_kernel_scores(A, B, da, kind, i, drop_last_column=False):
    """Row i of the score matrix in the arithmetic of eval.hip's RowScore (the one row score of the AP and top-k kernels): lane l sums the terms of columns l, l + 64, ... in fp64 in that order,
    wave_sum_f64 folds the 64 partial sums by the butterfly 32, 16, ..., 1.  drop_last_column plants a tail mask that is one short."""
    width = da - 1 if drop_last_column else da
    a = A[i, :width].astype(np.float64); b = (A if B is None else B)[:, :width].astype(np.float64)
    t = a[None, :] * b if kind == 0 else (a[None, :] - b) ** 2
    c = max((width + 63) // 64, 1)
    tp = np.zeros((t.shape[0], c * 64)); tp[:, :width] = t
    tp = tp.reshape(-1, c, 64)
    part = np.zeros((t.shape[0], 64))
    for k in range(c):
        part = part + tp[:, k, :]
    for o in (32, 16, 8, 4, 2, 1):
        part = part[:, :o] + part[:, o:2 * o]
    s = part[:, 0]
    if kind == 1:
        r = np.sqrt(s); s = np.exp(-(r * r))
    return s


def ap_by_counts(s, i, row, undirected, drop_last_neighbour=False):
    """gemhip_eval_ap's formula on one row of scores: the true neighbours t != i (t > i when undirected), each once; AP = mean over those
    with s_t > 0 of rank_hit / rank_all, both under the stable rule (score descending, id ascending)."""
    n = s.shape[0]
    nb = np.unique([t for t in row if t != i and not (undirected and t < i)]).astype(np.int64)
    if drop_last_neighbour:
        nb = nb[:-1]
    cand = np.arange(i + 1 if undirected else 0, n)
    cand = cand[(cand != i) & (s[cand] > 0)]
    nb = nb[s[nb] > 0]
    if nb.size == 0:
        return 0.0
    order = nb[np.lexsort((nb, -s[nb]))]
    total = 0.0
    for r, t in enumerate(order):
        ahead = int(np.sum((s[cand] > s[t]) | ((s[cand] == s[t]) & (cand < t))))
        total += (r + 1) / (1 + ahead)
    return total / nb.size


# ====================================================================================================================== GF objective
GF_U = 2.0 ** -24                     # unit roundoff of fp32
GF_WAVES = 2048 * 256 // 64           # wavefronts of gf_objective_kernel's fixed grid
GF_D = (1, 2, 63, 64, 65, 128, 130, 1024)
GF_M = (1, 8191, 8192, 8193)
GF_CASES = ['d%d' % d for d in GF_D] + ['m%d' % m for m in GF_M] + ['m0', 'n1', 'n8200', 'w_null', 'cancel']


def gf_case(name):
    """(n, src, dst, w, d, X) of one case.  Edge 0 is a self-loop, edge 1 has dst < src and edge 2 repeats it (the objective runs over ALL edges,
    gf.cpp:94-113); weights are uniform in (-2, 2) with one in ten set to zero, the last edge's is 3 so that losing it is visible;
    'cancel': w_e = float32(fp64 X_i.X_j), every residual at rounding level."""
    n, m, d = 300, 3000, 65
    if name[0] == 'd':
        d = int(name[1:])
    elif name[0] == 'm':
        m = int(name[1:])
    elif name == 'n1':
        n, m = 1, 3
    elif name == 'n8200':
        n, d = 8200, 2
    elif name == 'w_null':
        d = 64
    elif name == 'cancel':
        d = 130
    rng = np.random.RandomState(1000 + GF_CASES.index(name))
    src = rng.randint(0, n, m).astype(np.int32); dst = rng.randint(0, n, m).astype(np.int32)
    if m >= 3 and n > 9:
        src[:3] = [7, 9, 9]; dst[:3] = [7, 3, 3]
    X = (rng.randn(n, d) * 0.5 / d ** 0.25).astype(np.float32)                    # |X_i.X_j| of order 1/4 at every d
    w = rng.uniform(-2, 2, m).astype(np.float32)
    w[rng.rand(m) < 0.1] = 0.0
    if m:
        w[-1] = 3.0
    if name == 'w_null':
        w = None
    if name == 'cancel':
        w = (X[src].astype(np.float64) * X[dst].astype(np.float64)).sum(axis=1).astype(np.float32)
    return n, src, dst, w, d, X


def gf_reference_and_bound(n, src, dst, w, d, X):
    """fp64 f1, f2 and the bounds on what gf_objective_kernel may return.  The kernel's dot product passes every term through one product rounding
    (none under FMA contraction), ceil(d/64) - 1 fp32 additions in its lane and the 6 levels of wave_sum: with L = ceil(d/64) + 7,
    |dot - X_i.X_j| <= L u sum_k |x_ik x_jk|, and the fp32 subtraction from w adds u |r|:  delta_e = L u sum_k |x_ik x_jk| + u |r_e|.
    |r~^2 - r^2| <= delta (2|r| + delta); the fp64 accumulation of m (n) terms in any order adds m 2^-50 f1 (n 2^-50 f2).  Every term of
    f2 is non-negative, so its fp32 part is relative: L u f2."""
    L = (d + 63) // 64 + 7
    X64 = X.astype(np.float64)
    xi, xj = X64[src], X64[dst]
    r = (np.ones(len(src)) if w is None else w.astype(np.float64)) - (xi * xj).sum(axis=1)
    delta = L * GF_U * np.abs(xi * xj).sum(axis=1) + GF_U * np.abs(r)
    f1 = float((r * r).sum()); f2 = float((X64 * X64).sum())
    b1 = float((delta * (2 * np.abs(r) + delta)).sum()) + len(src) * 2.0 ** -50 * f1
    b2 = (L * GF_U + n * 2.0 ** -50) * f2
    return f1, f2, b1, b2


def _wave_sum_f32(part):
    """common.hpp wave_sum on [rows][64] float32: neighbours, pairs, quads, eights (the four DPP steps), then (r0 + r1) + (r2 + r3)."""
    for _ in range(6):
        part = part[:, 0::2] + part[:, 1::2]
    assert part.dtype == np.float32
    return part[:, 0]


def _lane_dots_f32(a, b, fma):
    rows, d = a.shape
    c = (d + 63) // 64
    ap = np.zeros((rows, c * 64), np.float32); bp = np.zeros((rows, c * 64), np.float32)
    ap[:, :d] = a; bp[:, :d] = b
    ap = ap.reshape(rows, c, 64); bp = bp.reshape(rows, c, 64)
    part = np.zeros((rows, 64), np.float32)
    for k in range(c):                                                             # `for (k = lane; k < d; k += 64) part += xi[k] * xj[k]`
        if fma:
            part = (ap[:, k].astype(np.float64) * bp[:, k].astype(np.float64) + part.astype(np.float64)).astype(np.float32)
        else:
            part = part + ap[:, k] * bp[:, k]
    return _wave_sum_f32(part)


def gf_emulate(n, src, dst, w, d, X, fma=False, drop_edge=None, drop_last_column=False, drop_node=None):
    """gf_objective_kernel's own arithmetic in numpy: fp32 lane sums and wave_sum, r in fp32, r*r and every further sum in fp64, a wavefront
    summing its edges e = wave, wave + 8192, ... in order and the wavefronts' sums added one after another (the atomics' order is free: the
    bound's m 2^-50 term covers any).  The three planted mistakes: an edge lost, a tail mask one short, a node's norm lost."""
    dd = d - 1 if drop_last_column else d
    Xd = np.ascontiguousarray(X[:, :dd]) if dd else np.zeros((n, 1), np.float32)
    e = np.arange(len(src))
    if drop_edge is not None:
        e = e[e != drop_edge]
    wv = np.ones(len(e), np.float32) if w is None else w[e]
    r = wv - _lane_dots_f32(Xd[src[e]], Xd[dst[e]], fma)
    assert r.dtype == np.float32
    f1 = float(np.bincount(e % GF_WAVES, weights=r.astype(np.float64) ** 2, minlength=1).sum()) if len(e) else 0.0
    v = np.arange(n)
    if drop_node is not None:
        v = v[v != drop_node]
    f2 = float(np.bincount(v % GF_WAVES, weights=_lane_dots_f32(Xd[v], Xd[v], fma).astype(np.float64), minlength=1).sum())
    return f1, f2


# ====================================================================================================================== HOPE SVD error
SVD_BAR = 5e-3                        # relative, against the dense value: six s.d. of the 32-probe estimate (measured: tests/README.md)
SVD_SBM_K = ((130, 129), (160, 150), (256, 200))         # k and the second-chunk column of U that the test halves
SVD_ASYM_K = 136


def operator_arrays(n, src, dst, w, order):
    """Edge arrays by POSITION in graph.nodes (hope.py:28 indexes rows that way), float32 weights, and the dense fp64 A of those weights."""
    if order is not None:
        pos = np.empty(n, dtype=np.int64); pos[np.asarray(order)] = np.arange(n)
        src, dst = pos[src], pos[dst]
    src = np.asarray(src, dtype=np.int32); dst = np.asarray(dst, dtype=np.int32)
    w = np.ones(len(src), np.float32) if w is None else np.asarray(w, dtype=np.float32)
    A = np.zeros((n, n)); A[src, dst] = w.astype(np.float64)
    return src, dst, w, A


def katz_dense(A, beta):
    """hope.py:29-31: S = (I - beta A)^-1 beta A in fp64, from the fp32-rounded weights the device holds."""
    n = A.shape[0]
    return np.linalg.solve(np.eye(n) - beta * A, beta * A)


def asym_graph():
    """A weighted directed graph on 400 nodes whose out- and in-degrees follow different laws (sources from a skewed draw, targets uniform),
    weights in (0, 2), beta with beta ||A||_2 ~ 0.5.  Returns (n, src, dst, w float32, beta, A dense fp64 of the float32 weights)."""
    n = 400
    rng = np.random.RandomState(77)
    src = np.minimum((n * rng.rand(6000) ** 2.5).astype(np.int64), n - 1); dst = rng.randint(0, n, 6000)
    key = np.unique(src * n + dst)
    key = key[key // n != key % n]
    src, dst = (key // n).astype(np.int32), (key % n).astype(np.int32)
    w = (2.0 * (1.0 - rng.rand(len(src)))).astype(np.float32)
    w = np.maximum(w, np.float32(1e-3))
    A = np.zeros((n, n)); A[src, dst] = w.astype(np.float64)
    beta = float(np.float32(0.5 / np.linalg.norm(A, 2)))
    return n, src, dst, w, beta, A


def svd_inputs(u, s, vt, k):
    """What a solve returns, from the dense SVD rounded to fp32: sigma, U sqrt(Sigma), V sqrt(Sigma) ([n][k], row-major)."""
    sig = np.ascontiguousarray(s[:k], dtype=np.float32)
    rt = np.sqrt(sig.astype(np.float64))
    return sig, np.ascontiguousarray(u[:, :k] * rt, dtype=np.float32), np.ascontiguousarray(vt[:k].T * rt, dtype=np.float32)


def svd_error_dense(S, sig, U_sqrtS, V_sqrtS):
    """hope.py:38-40 on the factorisation the device is handed: ||u diag(s) vt - S||_F with u diag(s) vt = (U sqrt(s)) (V sqrt(s))^T."""
    return float(np.linalg.norm(U_sqrtS.astype(np.float64) @ V_sqrtS.astype(np.float64).T - S))


def svd_uside_dense(S, sig, U_sqrtS, V_sqrtS, columns=None):
    """||S V - U Sigma||_F over unit V; `columns` restricts it (a chunk loop that stops early sees only those)."""
    rt = np.sqrt(sig.astype(np.float64))
    R = S @ (V_sqrtS.astype(np.float64) / rt) - U_sqrtS.astype(np.float64) * rt
    return float(np.linalg.norm(R if columns is None else R[:, :columns]))


def svd_trunc_estimates(B, S, V, Z, probes=32, bv_columns=None):
    """svd_error_impl's truncation estimate restated in fp64, for every group of `probes` columns of the normal matrix Z at once:
    trunc^2 = ||B||_F^2 - ||B V||_F^2 + mean_z (||S P z||^2 - ||B P z||^2),  P z = z - V V^T z  (B = beta A, the first Katz term, kept exact).
    bv_columns plants a B V loop that stops after that many columns.  Returns the estimates of trunc (one per group)."""
    BV = B @ V
    bv2 = float((BV[:, :bv_columns] ** 2).sum())
    C = V.T @ Z
    SZ = S @ Z - (S @ V) @ C
    BZ = B @ Z - BV @ C
    rem = ((SZ * SZ).sum(axis=0) - (BZ * BZ).sum(axis=0)).reshape(-1, probes).mean(axis=1)
    return np.sqrt(np.maximum(0.0, float((B * B).sum()) - bv2 + rem))
