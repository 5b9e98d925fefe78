"""Device-free references, inputs and bounds for the layer between HOPE's launch functions and its solvers:

  apply_S / apply_ST                  (gem_amd/csrc/hope_ops.hip)     the Katz series, (I + M) X, c X - N^T N X
  cheb_filter                         (gem_amd/csrc/hope_solve.hip)   three-term recurrence, fused epilogue, in-filter projection
  orth / orth_scaled via orth_passes  (hope_solve.hip, hope_ops.hpp)  Y <- Y C through Tmp, a column count that shrinks
  katz_rho_estimate, lle_shift_estimate (gem_amd/csrc/hope.hip)       the spectrum estimates of the two set-ups

test_hope_operators_gpu.py holds the device against these through the gemhip_test_hope_apply_s / _cheb_filter / _orth / _spectrum_estimate
hooks; test_hope_operator_refs.py holds, without a device, a numpy float32 emulation of each composition (the same sequence of
SpMM-with-epilogue steps) inside every bound at every shape the GPU tests use, and shows that each planted mistake leaves it by more than ten bounds.

The bounds are error recurrences of the iterations themselves, in the style of test_hope_blocks_gpu.spmm_ref: a step Y = alpha A X + sum_k w_k W_k
on inputs that carry the errors E_X, E_k is within
    |alpha| |A| E_X + sum_k |w_k| E_k  +  (deg + 4) 2^-23 (|alpha| |A| |X| + sum_k |w_k| |W_k|)
of the fp64 step, elementwise, |X| and |W_k| being the fp64 reference's own iterates; a step whose inputs carry errors gets the factor 1.01 for
the second-order terms (the magnitudes are the reference's, not the device's)."""
import os

import numpy as np
import scipy.sparse as sp

import instrument_refs as ir
from hope_sym_mirror import _orth_scaled
from test_hope_blocks_gpu import make_graph, stochastic_graph          # (imports no device: gem_amd._hip loads the library on first use)

U = 2.0 ** -23
WIDE = 10.0                     # a planted mistake leaves the bound by more than this many bounds
SECOND_ORDER = 1.01
HERE = os.path.dirname(os.path.abspath(__file__))


def f32(x):
    return float(np.float32(x))


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound, elementwise (a bound of exactly 0 -- an empty row -- must be met exactly)."""
    err = np.abs(np.asarray(out, np.float64) - ref)
    return float(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max())


# ====================================================================================================================== one SpMM step
def op_of(g, transpose=False):
    """(A, |A|, row degrees) of a test_hope_blocks_gpu graph, or of its transpose (the CSR the device builds for spmm(H, true, ...))."""
    if not transpose:
        return g['A'], g['absA'], g['deg']
    AT = g['A'].T.tocsr()
    return AT, abs(AT), np.asarray((g['A'] != 0).sum(axis=0)).ravel().astype(np.float64)


def step64(op, alpha, X, EX, adds=()):
    """(fp64 value, elementwise bound) of alpha A X + sum coef W: X carries the error EX, adds = [(coef, W, EW)] (EW None: exact)."""
    A, aA, deg = op
    ref = alpha * (A @ X); mag = abs(alpha) * (aA @ np.abs(X)); prop = abs(alpha) * (aA @ EX) if EX is not None else 0.0
    exact = EX is None
    for coef, W, EW in adds:
        ref = ref + coef * W; mag = mag + abs(coef) * np.abs(W)
        if EW is not None:
            prop = prop + abs(coef) * EW; exact = False
    E = prop + (deg[:, None] + 4) * U * mag
    return ref, E if exact else SECOND_ORDER * E


def step32(A32, alpha, X, adds=()):
    """The same step in numpy float32: the row's products summed in CSR order, then the epilogue."""
    out = np.float32(alpha) * (A32 @ X)
    for coef, W in adds:
        out = out + np.float32(coef) * W
    assert out.dtype == np.float32
    return out


def csr32(g, transpose=False):
    A = sp.csr_matrix((g['va'], g['ci'].copy(), g['rp'].copy()), shape=(g['n'], g['n']))
    return A.T.tocsr() if transpose else A


# ====================================================================================================================== apply_S / apply_ST
S_TERMS = (0, 1, 2, 3, 4, 7)
S_WIDTHS = (1, 16, 17, 96, 130)
_katz = {}


def katz_graph(n):
    """make_graph(n) as test_hope_blocks_gpu.graph(n) seeds it (n = 203: signed, directed, crafted degrees; n = 1: a self loop) and the
    float32 beta with beta ||A||_2 = 0.5."""
    if n not in _katz:
        g = make_graph(n, 7 + n)
        _katz[n] = (g, f32(0.5 / np.linalg.norm(g['A'].toarray(), 2)))
    return _katz[n]


def s_input(n, b, transpose):
    return np.random.RandomState(31 * b + transpose + n).randn(n, b).astype(np.float32)


def katz_dense_series(g, beta, terms, transpose):
    """sum_{t = 1 .. terms + 1} (beta A)^t, or its transpose, as a dense fp64 matrix."""
    B = beta * g['A'].toarray()
    S = np.zeros_like(B); P = np.eye(g['n'])
    for _ in range(terms + 1):
        P = P @ B; S = S + P
    return S.T if transpose else S


def apply_s_bound(g, beta, X, terms, transpose):
    """The error recurrence of the iteration apply_S / apply_ST runs (mode 0).  apply_S: W0 = beta A X (E_0 = (deg + 4) u M_0), then
    Z <- beta A Z + W0, `terms` times:  E_{t+1} = 1.01 (|beta| |A| E_t + (deg + 4) u (|beta| |A| M_t + M_0)),  M_t = |Z_t|, M_0 = |W0| of the fp64
    iteration (the recurrence as the operator tests state it: W0's own error E_0 is not carried through the addend a second time).
    apply_ST: R <- Y + beta A^T R from R = Y, `terms` times, then Z = beta A^T R; Y is exact."""
    X = X.astype(np.float64)
    if not transpose:
        op = op_of(g)
        Z, E = step64(op, beta, X, None)
        W0 = Z
        for _ in range(terms):
            Z, E = step64(op, beta, Z, E, [(1.0, W0, None)])
        return Z, E
    op = op_of(g, True)
    R, E = X, None
    for _ in range(terms):
        R, E = step64(op, beta, R, E, [(1.0, X, None)])
    return step64(op, beta, R, E)


def apply_s_emulate(g, beta, X, terms, transpose, use_transposed_matrix=None):
    """apply_S / apply_ST of mode 0 in float32.  use_transposed_matrix overrides which CSR the steps read (the planted A^T for A)."""
    A32 = csr32(g, transpose if use_transposed_matrix is None else use_transposed_matrix)
    if not transpose:
        W0 = step32(A32, beta, X)
        Z = W0
        for _ in range(terms):
            Z = step32(A32, beta, Z, [(1.0, W0)])
        return Z
    R = X
    for _ in range(terms):
        R = step32(A32, beta, R, [(1.0, X)])
    return step32(A32, beta, R)


def mode1_ref(g, X):
    """(I + M) X: one step with Wadd = X."""
    return step64(op_of(g), 1.0, X.astype(np.float64), None, [(1.0, X.astype(np.float64), None)])


def mode2_ref(g, c, X):
    """c X - N^T N X, N = I - P, as apply_S runs it: W0 = X - P X, T0 = P^T W0, Out = c X - W0 + T0 (a three-flop lincomb)."""
    X = X.astype(np.float64)
    W0, E0 = step64(op_of(g), -1.0, X, None, [(1.0, X, None)])
    T0, ET = step64(op_of(g, True), 1.0, W0, E0)
    ref = c * X - W0 + T0
    return ref, SECOND_ORDER * (E0 + ET + 3 * U * (abs(c) * np.abs(X) + np.abs(W0) + np.abs(T0)))


def mode2_emulate(g, c, X):
    W0 = step32(csr32(g), -1.0, X, [(1.0, X)])
    T0 = step32(csr32(g, True), 1.0, W0)
    return np.float32(c) * X - W0 + T0


# ====================================================================================================================== cheb_filter
F_COLS = (5, 33)
F_DEGREES = (1, 2, 3, 4, 7)
F_LOCKED = [(4, 2), (4, 3), (7, 2), (7, 3)]          # (m, q) with nl = 3
# e over half the spectrum's width.  The error recurrence grows by up to 2 || |Op| || / e + 2 |c| / e + 1 per degree whatever the polynomial does, so at
# e = half the width it has grown past the planted mistakes by degree 7 (kind 2, where |Op| = (I + |P|)^T (I + |P|): past the result itself); a wider
# interval -- a smaller ||Op|| / e -- keeps the same recurrence, coefficients and schedule and lets the bound tell them apart (test_hope_operator_refs.py)
F_STRETCH = {0: 3.0, 2: 12.0}
_filter = {}


def sym_graph(n=203, seed=11):
    """A symmetric weighted graph: positive fp32 weights, a hub of 60 neighbours, one isolated node, unsorted rows."""
    rng = np.random.RandomState(seed)
    i = rng.randint(0, n - 1, 900); j = rng.randint(0, n - 1, 900)
    i = np.concatenate([i, np.zeros(60, np.int64)]); j = np.concatenate([j, rng.choice(np.arange(1, n - 1), 60, replace=False)])
    keep = i != j
    lo, hi = np.minimum(i, j)[keep], np.maximum(i, j)[keep]
    key = np.unique(lo * n + hi)
    lo, hi = key // n, key % n
    w = (rng.rand(len(key)) + 0.1).astype(np.float32)
    A = sp.coo_matrix((np.concatenate([w, w]).astype(np.float64), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))), shape=(n, n)).tocsr()
    return _graph_dict(A, rng)


def _graph_dict(A, rng=None):
    """The dictionary of test_hope_blocks_gpu.make_graph for a scipy CSR matrix of fp32-representable values (rows shuffled when rng is given)."""
    n = A.shape[0]
    A = A.tocsr(); A.sort_indices()
    rp = A.indptr.astype(np.int64); ci = A.indices.astype(np.int32).copy(); va = A.data.astype(np.float32).copy()
    if rng is not None:
        for r in range(n):
            p = rng.permutation(rp[r + 1] - rp[r])
            ci[rp[r]:rp[r + 1]] = ci[rp[r]:rp[r + 1]][p]; va[rp[r]:rp[r + 1]] = va[rp[r]:rp[r + 1]][p]
    A64 = sp.csr_matrix((va.astype(np.float64), ci.copy(), rp.copy()), shape=(n, n))
    return dict(n=n, rp=rp, ci=ci, va=va, A=A64, absA=abs(A64), deg=np.diff(rp).astype(np.float64))


def row_normalised(g):
    """P = D^-1 A with the fp32 values lle_edge_values produces: float32(w / l1) per row."""
    va = g['va'].astype(np.float64).copy()
    for r in range(g['n']):
        s = np.abs(va[g['rp'][r]:g['rp'][r + 1]]).sum()
        va[g['rp'][r]:g['rp'][r + 1]] = va[g['rp'][r]:g['rp'][r + 1]] / s if s > 0 else 0.0
    va = va.astype(np.float32)
    A = sp.csr_matrix((va.astype(np.float64), g['ci'].copy(), g['rp'].copy()), shape=(g['n'], g['n']))
    return dict(n=g['n'], rp=g['rp'], ci=g['ci'], va=va, A=A, absA=abs(A), deg=g['deg'])


def filter_case(kind):
    """(graph, dense Op, eigenvalues ascending, eigenvectors) of a kind: 0: Op = A (symmetric); 2: Op = (I - P)^T (I - P), P = D^-1 A."""
    if kind not in _filter:
        g = sym_graph() if kind == 0 else row_normalised(sym_graph())
        D = g['A'].toarray()
        Op = D if kind == 0 else (np.eye(g['n']) - D).T @ (np.eye(g['n']) - D)
        lam, Z = np.linalg.eigh(0.5 * (Op + Op.T))
        _filter[kind] = (g, Op, lam, Z)
    return _filter[kind]


def filter_interval(kind, where):
    """(c, e): 'inside': the whole spectrum within [c - e, c + e] (2 % to spare); 'outside': the top eigenvalue 10 % of e above c + e."""
    lam = filter_case(kind)[2]
    lo, hi = lam[0], lam[-1]
    e = F_STRETCH[kind] * 0.5 * (hi - lo)
    if where == 'inside':
        return 0.5 * (hi + lo), e
    return hi - 1.1 * e, e                            # c + 1.1 e = hi


def filter_input(kind, cols):
    return np.random.RandomState(100 * kind + cols).randn(203, cols).astype(np.float32)


def locked_block(kind, nl=3):
    """The nl top eigenvectors of the dense operator, rounded to fp32."""
    return np.ascontiguousarray(filter_case(kind)[3][:, ::-1][:, :nl], dtype=np.float32)


def _sym_step64(kind, g, alpha, X, EX, adds):
    """apply_sym_op in fp64 with its bound.  kind 0: one SpMM step.  kind 2: T = X - P X; Z = sum coef W (a lincomb: 3 u |Z|); Out = alpha (T - P^T T) + Z."""
    if kind == 0:
        return step64(op_of(g), alpha, X, EX, adds)
    T, ET = step64(op_of(g), -1.0, X, EX, [(1.0, X, EX)])
    if not adds:
        return step64(op_of(g, True), -alpha, T, ET, [(alpha, T, ET)])
    Z = sum(coef * W for coef, W, _ in adds); aZ = sum(abs(coef) * np.abs(W) for coef, W, _ in adds)
    EZ = sum(abs(coef) * (EW if EW is not None else 0.0) for coef, W, EW in adds) + 3 * U * aZ
    return step64(op_of(g, True), -alpha, T, ET, [(alpha, T, ET), (1.0, Z, EZ)])


def _sym_step32(kind, g, alpha, X, adds):
    if kind == 0:
        return step32(csr32(g), alpha, X, adds)
    T = step32(csr32(g), -1.0, X, [(1.0, X)])
    if not adds:
        return step32(csr32(g, True), -alpha, T, [(alpha, T)])
    Z = None
    for coef, W in adds:
        Z = np.float32(coef) * W if Z is None else Z + np.float32(coef) * W
    return step32(csr32(g, True), -alpha, T, [(alpha, T), (1.0, Z)])


def _project64(Q, W, EW):
    """W - Q (Q^T W) with test_hope_blocks_gpu's project_out bound: the fp32 coefficients are within e1 = (n + 1) u |Q|^T |W| of Q^T W, the GEMM adds
    (nl + 2) u (|W| + |Q| (|Q^T W| + e1)); an input error passes through I + |Q| |Q|^T."""
    n, nl = Q.shape
    G = Q.T @ W
    e1 = (n + 1) * U * (np.abs(Q).T @ np.abs(W))
    local = np.abs(Q) @ e1 + (nl + 2) * U * (np.abs(W) + np.abs(Q) @ (np.abs(G) + e1))
    if EW is None:
        return W - Q @ G, local
    return W - Q @ G, SECOND_ORDER * (EW + np.abs(Q) @ (np.abs(Q).T @ EW) + local)


def _project32(Q, W):
    G = (Q.astype(np.float64).T @ W.astype(np.float64)).astype(np.float32)            # fp64 slab reduction, one rounding to fp32
    return W - Q @ G


def cheb_coefficients(c, e):
    """The float32 scalars cheb_filter hands to the epilogue: (1/e, -c/e) of degree 1, (2/e, -2c/e) of the recurrence."""
    return f32(1.0 / e), f32(-c / e), f32(2.0 / e), f32(-2.0 * c / e)


def cheb_ref(kind, V, m, c, e, Q=None, q=0):
    """(fp64 value, elementwise bound) of T_m((Op - c) / e) V by the three-term recurrence, V as Y_0; with Q, both live terms are projected before
    degree j whenever (j - 1) % q == 0 (j >= 2) -- the schedule cheb_filter's comment states."""
    g = filter_case(kind)[0]
    a1, w1, a2, w2 = cheb_coefficients(c, e)
    Q64 = None if Q is None else Q.astype(np.float64)
    Y0, E0 = V.astype(np.float64), None
    Y1, E1 = _sym_step64(kind, g, a1, Y0, None, [(w1, Y0, None)])
    for j in range(2, m + 1):
        if Q64 is not None and q > 0 and (j - 1) % q == 0:
            Y0, E0 = _project64(Q64, Y0, E0); Y1, E1 = _project64(Q64, Y1, E1)
        Y2, E2 = _sym_step64(kind, g, a2, Y1, E1, [(w2, Y1, E1), (-1.0, Y0, E0)])
        Y0, E0, Y1, E1 = Y1, E1, Y2, E2
    return Y1, E1


def cheb_dense(kind, V, m, c, e):
    """The same polynomial from the dense operator (the recurrence on matrices): what cheb_ref must equal without locked vectors."""
    Op = filter_case(kind)[1]
    a1, w1, a2, w2 = cheb_coefficients(c, e)
    V = V.astype(np.float64)
    Y0, Y1 = V, a1 * (Op @ V) + w1 * V
    for _ in range(2, m + 1):
        Y0, Y1 = Y1, a2 * (Op @ Y1) + w2 * Y1 - Y0
    return Y1


def cheb_emulate(kind, V, m, c, e, Q=None, q=0, mistake=None):
    """cheb_filter in float32, with one planted mistake: 'half_c' (-c/e for -2c/e), 'y0' (V as Y_{j-1} at degree 3), 'skip' (no projection),
    'one_term' (only the newer live term projected), 'late' (the projection one degree late)."""
    g = filter_case(kind)[0]
    a1, w1, a2, w2 = cheb_coefficients(c, e)
    if mistake == 'half_c':
        w2 = w1
    Y0 = V
    Y1 = _sym_step32(kind, g, a1, V, [(w1, V)])
    for j in range(2, m + 1):
        due = (j - 2) % q == 0 and j >= 3 if (mistake == 'late' and q > 0) else (q > 0 and (j - 1) % q == 0)
        if Q is not None and due and mistake != 'skip':
            if mistake != 'one_term':
                Y0 = _project32(Q, Y0)
            Y1 = _project32(Q, Y1)
        Y2 = _sym_step32(kind, g, a2, Y1, [(w2, Y1), (-1.0, V if (mistake == 'y0' and j == 3) else Y0)])
        Y0, Y1 = Y1, Y2
    return Y1


# ====================================================================================================================== orth / orth_scaled
ORTH_N = (203, 1500)
ORTH_B = (3, 32, 33, 96)
ORTH_CASES = ('gaussian', 'graded', 'duplicate', 'zero')
# orth's (tol, abs_floor) per case (the solvers pass 1e-9 ... 1e-11, later passes 1e-12, and 1e-12 x an energy).  graded: the squared norms span
# 1e-6 and a 203 x 96 Gaussian block another 1e-2, so only tol = 1e-12 leaves its smallest direction 1e4 above the threshold; nothing is dropped there
ORTH_ARGS = {'gaussian': (1e-10, 0.0), 'graded': (1e-12, 0.0), 'duplicate': (1e-10, 0.0), 'zero': (1e-10, 1e-6)}
ORTH_BAR_FACTOR = 4.0                          # device ||Y^T Y - I||_max against the float32 restatement's: summation order and FMA contraction


def orth_input(n, b, case, scaled):
    """(Y float32 [n][b], constructed rank).  graded: column norms 1 ... 1e-3 of the Gaussian's; duplicate: the last column repeats column 0;
    zero: column 1 is zero and, for orth, column 2 (the last one at b = 3) has energy 1e-12, 1e6 below abs_floor = 1e-6.  Every dropped direction
    is >= 1e4 under its threshold, every kept one >= 1e4 above (test_hope_operator_refs.py computes both)."""
    Y = np.random.RandomState(n + 7 * b + ORTH_CASES.index(case)).randn(n, b)
    rank = b
    if case == 'graded':
        Y = Y * np.logspace(0, -3, b)
    elif case == 'duplicate':
        Y[:, -1] = Y[:, 0]; rank = b - 1
    elif case == 'zero':
        Y[:, 1] = 0.0; rank = b - 1
        if not scaled:
            Y[:, 2] *= 1e-6 / np.linalg.norm(Y[:, 2]); rank = b - 2
    return Y.astype(np.float32), rank


def _chol_coefficients(G, floor):
    """C = R^-1 of G = R^T R, or None when a pivot is not above `floor` (chol_inverse)."""
    try:
        R = np.linalg.cholesky(G).T
    except np.linalg.LinAlgError:
        return None
    if not np.all(np.diag(R) ** 2 > floor):
        return None
    return np.linalg.inv(R)


def orth_unscaled(Y, tol, abs_floor, passes=2):
    """orth() restated (orth_pass: Cholesky unless a pivot is under max(1e-4 dmax, abs_floor), else the Gram matrix's eigenvectors above tol lmax and
    abs_floor; later passes with tol = 1e-12, abs_floor = 0), float32 blocks and fp64 small matrices: _orth_scaled's unscaled sibling."""
    for _ in range(passes):
        if Y.shape[1] == 0:
            break
        G = (Y.T @ Y).astype(np.float64)
        C = _chol_coefficients(G, max(1e-4 * np.diag(G).max(), abs_floor))
        if C is None:
            w, Z = np.linalg.eigh(G)
            keep = (w > tol * max(w[-1], 0.0)) & (w > abs_floor) & (w > 0.0)
            C = Z[:, keep][:, ::-1] / np.sqrt(w[keep][::-1])
        Y = Y @ C.astype(np.float32)
        tol, abs_floor = 1e-12, 0.0
    return Y


def orth_restated(Y, case, scaled, passes=2):
    return _orth_scaled(Y, passes) if scaled else orth_unscaled(Y, ORTH_ARGS[case][0], ORTH_ARGS[case][1], passes)


def orth_defect(Y):
    Y = Y.astype(np.float64)
    return float(np.abs(Y.T @ Y - np.eye(Y.shape[1])).max()) if Y.shape[1] else 0.0


def span_residual(Yout, Yin):
    """max over columns of ||y - Yin x||_2 / ||y||_2, x the fp64 least-squares solution: how far span(Yout) leaves span(Yin)."""
    Yout = Yout.astype(np.float64); Yin = Yin.astype(np.float64)
    Yin = Yin[:, np.linalg.norm(Yin, axis=0) > 0]
    scale = np.linalg.norm(Yin, axis=0)
    x = np.linalg.lstsq(Yin / scale, Yout, rcond=1e-13)[0]
    return float((np.linalg.norm(Yout - (Yin / scale) @ x, axis=0) / np.linalg.norm(Yout, axis=0)).max())


def span_bound(Yin, b):
    """Y_out = (Y_in C1 + D1) C2 + D2 with |D| <= (b + 3) u |Y| |C| per tall-skinny GEMM (test_hope_blocks_gpu's bound); C2 polishes (~I), and a unit
    output column y = Y_in c has sum_k |Y_in[:, k]| |c_k| <= sqrt(b) ||y|| / s_min for column-normalised Y_in with smallest singular value s_min.
    Two passes: 2 (b + 3) u sqrt(b) / s_min, and the factor 1.01 for the second-order terms."""
    Yin = Yin.astype(np.float64)
    Yin = Yin[:, np.linalg.norm(Yin, axis=0) > 0]
    s = np.linalg.svd(Yin / np.linalg.norm(Yin, axis=0), compute_uv=False)
    smin = s[s > 1e-6 * s[0]].min()                  # of the directions that are there (a duplicated column adds an exact zero)
    return SECOND_ORDER * 2 * (b + 3) * U * np.sqrt(b) / smin


# ====================================================================================================================== spectrum estimates
EST_GRAPHS = ('sbm1024', 'asym400', 'star300', 'path500', 'signed_cliques', 'crafted203')
EST_UNDIRECTED = ('sbm1024', 'star300', 'path500', 'signed_cliques')
EST_SLACK = 1e-5
_est = {}


def _from_dense(A):
    A = sp.csr_matrix(A.astype(np.float32).astype(np.float64))
    return _graph_dict(A)


def estimate_graph(name):
    """The test_hope_blocks_gpu-style dictionary of one graph, with its dense fp64 matrix under 'dense'."""
    if name in _est:
        return _est[name]
    rng = np.random.RandomState(EST_GRAPHS.index(name))
    if name == 'sbm1024':                                       # the reference's SBM-1024 graph (tests/golden), nodes by position
        e = np.load(os.path.join(HERE, 'golden', 'sbm1024_edges.npy')); nodes = np.load(os.path.join(HERE, 'golden', 'sbm1024_nodes.npy'))
        pos = {int(v): k for k, v in enumerate(nodes.tolist())}
        A = np.zeros((len(nodes), len(nodes)))
        A[[pos[int(a)] for a in e[:, 0]], [pos[int(b)] for b in e[:, 1]]] = 1.0
    elif name == 'asym400':
        A = ir.asym_graph()[5]
    elif name == 'star300':                                     # node 0 with 300 leaves, inside a random graph of mean degree 4 on 1000 nodes
        n = 1000
        A = np.zeros((n, n))
        i = rng.randint(0, n, 2000); j = rng.randint(0, n, 2000)
        A[i[i != j], j[i != j]] = 1.0
        A[0, 1:301] = 1.0
        A = np.maximum(A, A.T)
    elif name == 'path500':
        n = 500
        A = np.zeros((n, n)); k = np.arange(n - 1)
        A[k, k + 1] = 1.0; A[k + 1, k] = 1.0
    elif name == 'signed_cliques':                              # D K_64 D with random signs D beside a plain K_32, weights 1, and 4 isolated nodes
        n = 100
        A = np.zeros((n, n))
        d = rng.choice([-1.0, 1.0], 64)
        A[:64, :64] = np.outer(d, d); A[64:96, 64:96] = 1.0
        np.fill_diagonal(A, 0.0)
    else:
        g = dict(make_graph(203, 7 + 203))
        g['dense'] = g['A'].toarray()
        _est[name] = g
        return g
    g = _from_dense(A)
    g['dense'] = g['A'].toarray()
    _est[name] = g
    return g


def hope_rho_window(g):
    """[lower, upper] for hope_setup's rho: sigma_max(A) (1 - 1e-5) <= rho <= min(1.1 sigma_max (1 + 1e-5), sqrt(max abs row sum x max abs column sum))."""
    D = g['dense']
    smax = float(np.linalg.norm(D, 2))
    cap = float(np.sqrt(np.abs(D).sum(axis=1).max() * np.abs(D).sum(axis=0).max()))
    return smax, smax * (1 - EST_SLACK), min(1.1 * smax * (1 + EST_SLACK), cap)


def lle_c_window(g):
    """[lower, upper] for gemhip_lle's c: sigma_max(I - P)^2 (1 - 1e-5) <= c <= 1.05 sigma_max^2 (1 + 1e-5), P the fp32 row-normalised matrix."""
    P = row_normalised(g)['A'].toarray()
    s2 = float(np.linalg.norm(np.eye(g['n']) - P, 2)) ** 2
    return s2, s2 * (1 - EST_SLACK), 1.05 * s2 * (1 + EST_SLACK)


def katz_terms(br):
    return max(1, min(int(np.ceil(np.log(1e-8) / np.log(br))) if br > 0 else 0, 400))


def power_iteration(apply_op, n, a, f, max_it, min_it, rel_tol, root_estimate):
    """hope_ops.hpp power_iteration restated in fp64 (the device's blocks are fp32, its norms fp64): ||Op x|| / ||x|| of the last step."""
    x = 1.0 + a * np.sin(f * (np.arange(n) + 1.0))
    x = x.astype(np.float32).astype(np.float64)
    ratio = est = 0.0
    steps = 0
    for it in range(max_it):
        z = apply_op(x)
        nx, nz = float(x @ x), float(z @ z)
        if not (nz > 0.0 and nx > 0.0 and np.isfinite(nz)):
            break
        prev = est
        ratio = np.sqrt(nz / nx)
        est = np.sqrt(ratio) if root_estimate else ratio
        x = z / np.sqrt(nz)
        steps = it + 1
        if it >= min_it and abs(est - prev) <= rel_tol * est:
            break
    return ratio, steps


def hope_rho_emulate(g):
    """katz_rho_estimate restated: (rho with margin and cap, rho before the cap, steps taken)."""
    D = g['dense']
    ratio, steps = power_iteration(lambda x: D.T @ (D @ x), g['n'], 0.37, 12.9898, 40, 4, 1e-3, True)
    cap = float(np.sqrt(np.abs(D).sum(axis=1).max() * np.abs(D).sum(axis=0).max()))
    raw = max(np.sqrt(ratio) * 1.1, 1e-30)
    return min(raw, cap), raw, steps


def lle_c_emulate(g):
    """lle_shift_estimate restated: (c, steps taken)."""
    N = np.eye(g['n']) - row_normalised(g)['A'].toarray()
    ratio, steps = power_iteration(lambda x: N.T @ (N @ x), g['n'], 0.61, 7.31, 60, 8, 1e-4, False)
    return (ratio * 1.05 if ratio > 0 else 4.0), steps
