"""GPU: the layer between HOPE's launch functions and its solvers, through the gemhip_test_hope_apply_s / _cheb_filter / _orth /
_spectrum_estimate hooks of include/gem_hip.h -- each calls the very function the solvers and set-ups call (apply_S / apply_ST, cheb_filter,
orth / orth_scaled, katz_rho_estimate / lle_shift_estimate).  A mistake here (a series term more or fewer, S^T that is not the transpose of S,
a wrong Chebyshev coefficient or start vector, a projection that is skipped, an estimate that ends under the true value) does not change what
the solvers converge to, only how close they get or how long they take: no end-to-end tolerance sees it.

Inputs, fp64 references and bounds are those of hope_operator_refs.py; test_hope_operator_refs.py shows without a device that a float32
emulation of each composition stays inside the bounds at these very shapes and that the planted mistakes leave them by more than ten bounds.
Every block with a leading dimension above its width carries test_hope_blocks_gpu's sentinel in the padding."""
import ctypes as C

import numpy as np
import pytest

import hope_operator_refs as hr
from gem_amd import _hip
from test_hope_blocks_gpu import SENT, assert_padding, fp, padded

pytestmark = pytest.mark.gpu


def csr(g):
    return g['n'], len(g['ci']), _hip.ptr(g['rp'], C.c_int64), _hip.ptr(g['ci'], C.c_int32), fp(g['va'])


def run_apply_s(g, mode, beta, transpose, terms, X, pads=(1, 2, 3)):
    """Out (n x ldo, sentinel outside the b columns) of apply_S / apply_ST with ldx, ldt, ldo = b + pads."""
    n, b = X.shape
    ldx, ldt, ldo = (b + p for p in pads)
    Out = np.full((n, ldo), SENT, np.float32)
    _hip.check(_hip.lib().gemhip_test_hope_apply_s(*csr(g), mode, beta, transpose, terms, b, fp(padded(X, ldx)), ldx, ldt, fp(Out), ldo))
    assert_padding(Out, 0, b)
    return Out


# ------------------------------------------------------------------------------------------------------------------ apply_S / apply_ST
@pytest.mark.parametrize('b', hr.S_WIDTHS)
@pytest.mark.parametrize('terms', hr.S_TERMS)
def test_katz_series_and_its_transpose(terms, b):
    """apply_S against dense fp64 sum_{t=1..terms+1} (beta A)^t X, apply_ST against the transpose of that matrix applied to Y: the copy path
    (terms = 0), Out as the last write after an odd and an even number of steps, both SpMM kernels (b = 130: one row per wavefront)."""
    for n in (203, 1):
        g, beta = hr.katz_graph(n)
        for transpose in (0, 1):
            X = hr.s_input(n, b, transpose)
            ref, E = hr.apply_s_bound(g, beta, X, terms, transpose)
            dense = hr.katz_dense_series(g, beta, terms, transpose) @ X.astype(np.float64)
            assert np.allclose(ref, dense, rtol=0, atol=1e-12 * np.abs(dense).max())
            Out = run_apply_s(g, 0, beta, transpose, terms, X)
            ratio = hr.worst_ratio(Out[:, :b], ref, E)
            print('%s n=%d terms=%d b=%d: max error / bound = %.3g' % ('apply_ST' if transpose else 'apply_S', n, terms, b, ratio))
            assert ratio <= 1.0


@pytest.mark.parametrize('b', hr.S_WIDTHS)
def test_laplacian_and_lle_operators_are_their_own_transposes(b):
    """Modes 1 and 2: (I + M) X and c X - N^T N X against fp64; apply_ST is the same launches on other scratch: bit for bit."""
    n = 203
    X = hr.s_input(n, b, 0)
    g = hr.katz_graph(n)[0]
    ref, E = hr.mode1_ref(g, X)
    S = run_apply_s(g, 1, 1.0, 0, 0, X); ST = run_apply_s(g, 1, 1.0, 1, 0, X)
    r1 = hr.worst_ratio(S[:, :b], ref, E)
    assert r1 <= 1.0 and np.array_equal(S.view(np.uint32), ST.view(np.uint32))
    p = hr.stochastic_graph(n, 5)
    c = hr.f32(3.3)
    ref, E = hr.mode2_ref(p, c, X)
    S = run_apply_s(p, 2, c, 0, 0, X); ST = run_apply_s(p, 2, c, 1, 0, X)
    r2 = hr.worst_ratio(S[:, :b], ref, E)
    print('b=%d: max error / bound = %.3g (mode 1), %.3g (mode 2)' % (b, r1, r2))
    assert r2 <= 1.0 and np.array_equal(S.view(np.uint32), ST.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ cheb_filter
def run_filter(kind, V, m, c, e, Q=None, q=0):
    g = hr.filter_case(kind)[0]
    n, cols = V.shape
    ldv, ldf = cols + 2, cols + 5
    Vp = padded(V, ldv)
    nl = 0 if Q is None else Q.shape[1]
    _hip.check(_hip.lib().gemhip_test_hope_cheb_filter(*csr(g), kind, m, c, e, fp(Vp), ldv, cols, ldf, None if Q is None else fp(padded(Q, nl + 2)), nl + 2,
                                                       nl, q))
    assert_padding(Vp, 0, cols)
    return Vp[:, :cols]


@pytest.mark.parametrize('cols', hr.F_COLS)
@pytest.mark.parametrize('where', ['inside', 'outside'])
@pytest.mark.parametrize('kind', [0, 2])
def test_chebyshev_filter_recurrence_and_coefficients(kind, where, cols):
    """T_m((Op - c) / e) V by the fp64 three-term recurrence on the dense operator: degree 1 (no recurrence step), 2 (V as Y_0), 3 and 4 (all three
    rotating blocks), 7; the whole spectrum inside [c - e, c + e], and the top eigenvalue 10 % of e above it."""
    c, e = hr.filter_interval(kind, where)
    V = hr.filter_input(kind, cols)
    for m in hr.F_DEGREES:
        ref, E = hr.cheb_ref(kind, V, m, c, e)
        dense = hr.cheb_dense(kind, V, m, c, e)
        assert np.allclose(ref, dense, rtol=0, atol=1e-11 * np.abs(dense).max())
        ratio = hr.worst_ratio(run_filter(kind, V, m, c, e), ref, E)
        print('kind %d %s cols=%d m=%d: max error / bound = %.3g' % (kind, where, cols, m, ratio))
        assert ratio <= 1.0


@pytest.mark.parametrize('cols', hr.F_COLS)
@pytest.mark.parametrize('m,q', hr.F_LOCKED)
@pytest.mark.parametrize('kind', [0, 2])
def test_chebyshev_filter_projects_locked_vectors_on_schedule(kind, m, q, cols):
    """Three dense eigenvectors (fp32) as Q, V random: both live terms lose Q before degree j whenever (j - 1) % q == 0."""
    c, e = hr.filter_interval(kind, 'inside')
    Q = hr.locked_block(kind)
    V = hr.filter_input(kind, cols)
    ref, E = hr.cheb_ref(kind, V, m, c, e, Q, q)
    out = run_filter(kind, V, m, c, e, Q, q)
    ratio = hr.worst_ratio(out, ref, E)
    Q64 = Q.astype(np.float64)
    left = np.abs(Q64.T @ out.astype(np.float64)); allowed = np.abs(Q64.T @ ref) + np.abs(Q64).T @ E
    print('kind %d m=%d q=%d cols=%d: max error / bound = %.3g; |Q^T V_out| <= %.3g against %.3g allowed' % (kind, m, q, cols, ratio, left.max(), allowed.max()))
    assert ratio <= 1.0
    assert np.all(left <= allowed)                                                 # what the last projection and the degrees after it leave of Q


# ------------------------------------------------------------------------------------------------------------------ orth / orth_scaled
@pytest.mark.parametrize('case', hr.ORTH_CASES)
@pytest.mark.parametrize('b', hr.ORTH_B)
@pytest.mark.parametrize('n', hr.ORTH_N)
@pytest.mark.parametrize('scaled', [0, 1])
def test_orthonormalisation_in_place_through_the_scratch_block(scaled, n, b, case):
    """orth / orth_scaled, two passes, ld = b + 3 and ldt = b + 5: the count kept is the constructed rank (it shrinks inside orth_passes for the
    duplicate and zero cases), the block stays inside span(Y_in), and ||Y^T Y - I||_max is within 4 x what the float32 restatement of the same
    passes leaves on the same input."""
    Y, rank = hr.orth_input(n, b, case, scaled)
    ld, ldt = b + 3, b + 5
    Yp = padded(Y, ld)
    keep = C.c_int32(-1)
    tol, floor = hr.ORTH_ARGS[case]
    _hip.check(_hip.lib().gemhip_test_hope_orth(n, fp(Yp), ld, b, ldt, scaled, tol, floor, 2, C.byref(keep)))
    assert_padding(Yp, 0, b)
    assert keep.value == rank
    Z = Yp[:, :rank]
    assert np.all(np.isfinite(Z))
    bar = hr.ORTH_BAR_FACTOR * hr.orth_defect(hr.orth_restated(Y, case, scaled))
    defect, res, res_bound = hr.orth_defect(Z), hr.span_residual(Z, Y), hr.span_bound(Y, b)
    print('%s n=%d b=%d %s: kept %d, ||Y^T Y - I||_max = %.3g (bar %.3g), span residual %.3g (bound %.3g)'
          % ('orth_scaled' if scaled else 'orth', n, b, case, rank, defect, bar, res, res_bound))
    assert res <= res_bound
    assert defect <= bar


# ------------------------------------------------------------------------------------------------------------------ spectrum estimates
@pytest.mark.parametrize('name', hr.EST_GRAPHS)
def test_set_up_estimates_against_dense_singular_values(name):
    """hope_setup's rho (power iteration on A^T A, x 1.1, capped by the absolute row / column sums) and gemhip_lle's c (on N^T N, x 1.05) against
    numpy's dense sigma_max; the br and the term count every solve reports (stats[7], stats[3]) are that rho's."""
    g = hr.estimate_graph(name)
    L = _hip.lib()
    smax, lo, hi = hr.hope_rho_window(g)
    rho = C.c_double(-1.0)
    _hip.check(L.gemhip_test_hope_spectrum_estimate(*csr(g), 0, C.byref(rho)))
    print('%s: rho %.6f = %.5f sigma_max(A), window [%.6f, %.6f]' % (name, rho.value, rho.value / smax, lo, hi))
    assert lo <= rho.value <= hi
    beta = hr.f32(0.5 / smax)
    plan = C.c_void_p()
    _hip.check(L.gemhip_hope_plan_create(*csr(g), beta, C.byref(plan)))
    try:
        n, k = g['n'], 4
        Uo = np.empty((n, k), np.float32); Vo = np.empty((n, k), np.float32); sig = np.empty(k, np.float32)
        stats = (C.c_double * 12)()
        _hip.check(L.gemhip_hope_plan_solve(plan, k, 16, 3, 20, 1e-5, 1, fp(Uo), fp(Vo), fp(sig), stats))
    finally:
        _hip.check(L.gemhip_hope_plan_destroy(plan))
    assert stats[7] == pytest.approx(beta * rho.value, rel=1e-12)
    assert stats[3] == hr.katz_terms(stats[7])
    if name in hr.EST_UNDIRECTED:
        s2, lo, hi = hr.lle_c_window(g)
        c = C.c_double(-1.0)
        _hip.check(L.gemhip_test_hope_spectrum_estimate(*csr(g), 1, C.byref(c)))
        print('%s: c %.6f = %.5f sigma_max(I - P)^2, window [%.6f, %.6f]' % (name, c.value, c.value / s2, lo, hi))
        assert lo <= c.value <= hi
