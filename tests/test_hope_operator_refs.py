"""CPU: the bounds of hope_operator_refs.py hold for a numpy float32 emulation of each composition (the same sequence of SpMM-with-epilogue,
projection and GEMM steps) at every shape test_hope_operators_gpu.py uses, and each planted mistake leaves them by more than ten bounds -- so
the GPU tests can fail.  Where a planted mistake cannot show at a shape, the test says why and asserts that reason:

  * one Katz term more or fewer at n = 203, terms = 4 and 7.  make_graph(203) is signed and directed: beta ||A||_2 = 0.5 but the spectral radius
    of beta A is 0.18, ||(beta A)^6||_2 = 1.4e-4 and ||(beta A)^9||_2 = 9e-7 -- at terms = 7 under the rounding bound of nine steps for ANY input
    (measured with the top singular vectors of that power as X: 2.4 and 11 bounds; random X: 1.0 and 7.2; apply_ST: 0.07 and 0.36), at terms = 4
    ten bounds clear for apply_S (> 190) but not at every width for apply_ST (9.3 ... 13).  The count is pinned at every `terms` by n = 1, where each
    term is worth 2^-t of the result (> 1000 bounds at terms = 7), and at n = 203 up to terms = 3.
  * the locked projection one degree late.  Q holds eigenvectors, so projecting commutes with the recurrence: a late projection that still
    precedes degree m gives the same block.  It shows exactly where the delay pushes the last projection past m: (m, q) = (4, 3)."""
import numpy as np
import pytest

import hope_operator_refs as hr

WIDE = hr.WIDE


# ------------------------------------------------------------------------------------------------------------------ apply_S / apply_ST
@pytest.mark.parametrize('n', [203, 1])
@pytest.mark.parametrize('terms', hr.S_TERMS)
def test_katz_series_bound_holds_and_planted_mistakes_break_it(n, terms):
    g, beta = hr.katz_graph(n)
    assert abs(beta * np.linalg.norm(g['A'].toarray(), 2) - 0.5) < 1e-6
    separable = n == 1 or terms <= 3
    for b in hr.S_WIDTHS:
        for transpose in (0, 1):
            X = hr.s_input(n, b, transpose)
            ref, E = hr.apply_s_bound(g, beta, X, terms, transpose)
            dense = hr.katz_dense_series(g, beta, terms, transpose) @ X.astype(np.float64)
            assert np.allclose(ref, dense, rtol=0, atol=1e-12 * np.abs(dense).max())              # the recurrence IS the dense series
            emu = hr.worst_ratio(hr.apply_s_emulate(g, beta, X, terms, transpose), ref, E)
            more = hr.worst_ratio(hr.apply_s_emulate(g, beta, X, terms + 1, transpose), ref, E)
            fewer = hr.worst_ratio(hr.apply_s_emulate(g, beta, X, terms - 1, transpose), ref, E) if terms else np.inf
            swapped = hr.worst_ratio(hr.apply_s_emulate(g, beta, X, terms, transpose, use_transposed_matrix=not transpose), ref, E)
            print('n=%d terms=%d b=%d %s: emulation %.3g of the bound; one term more %.3g, one fewer %.3g, the other CSR %.3g'
                  % (n, terms, b, 'apply_ST' if transpose else 'apply_S', emu, more, fewer, swapped))
            assert emu <= 1.0
            if n > 1:
                assert swapped > WIDE                                                             # A^T for A (n = 1: A^T = A)
            if separable:
                assert more > WIDE and fewer > WIDE                                               # (fewer at transpose = 1: apply_ST with terms - 1)
    if not separable:
        # why not: no input can make the dropped term stand ten bounds clear of nine steps' rounding at this graph
        B = beta * g['A'].toarray()
        assert np.abs(np.linalg.eigvals(B)).max() < 0.2 and np.linalg.norm(np.linalg.matrix_power(B, terms + 2), 2) < (2e-4 if terms == 4 else 1e-6)


@pytest.mark.parametrize('b', hr.S_WIDTHS)
def test_modes_1_and_2_bound_holds(b):
    n = 203
    g = hr.katz_graph(n)[0]
    X = hr.s_input(n, b, 0)
    ref, E = hr.mode1_ref(g, X)
    assert np.allclose(ref, X.astype(np.float64) + g['A'].toarray() @ X.astype(np.float64), rtol=0, atol=1e-12 * np.abs(ref).max())
    assert hr.worst_ratio(hr.step32(hr.csr32(g), 1.0, X, [(1.0, X)]), ref, E) <= 1.0
    p = hr.stochastic_graph(n, 5)
    c = hr.f32(3.3)
    ref, E = hr.mode2_ref(p, c, X)
    N = np.eye(n) - p['A'].toarray()
    assert np.allclose(ref, c * X.astype(np.float64) - N.T @ (N @ X.astype(np.float64)), rtol=0, atol=1e-12 * np.abs(ref).max())
    assert hr.worst_ratio(hr.mode2_emulate(p, c, X), ref, E) <= 1.0
    W0 = hr.step32(hr.csr32(p), -1.0, X, [(1.0, X)])
    assert hr.worst_ratio(np.float32(c) * X - W0 + hr.step32(hr.csr32(p), 1.0, W0), ref, E) > WIDE          # P for P^T in the second product


# ------------------------------------------------------------------------------------------------------------------ cheb_filter
@pytest.mark.parametrize('where', ['inside', 'outside'])
@pytest.mark.parametrize('kind', [0, 2])
def test_filter_bound_holds_and_planted_mistakes_break_it(kind, where):
    g, Op, lam, Z = hr.filter_case(kind)
    c, e = hr.filter_interval(kind, where)
    top = (lam[-1] - c) / e
    assert (lam[0] - c) / e >= -1.0 and (abs(top - 1.1) < 1e-12 if where == 'outside' else top <= 1.0)
    for cols in hr.F_COLS:
        V = hr.filter_input(kind, cols)
        for m in hr.F_DEGREES:
            ref, E = hr.cheb_ref(kind, V, m, c, e)
            dense = hr.cheb_dense(kind, V, m, c, e)
            assert np.allclose(ref, dense, rtol=0, atol=1e-11 * np.abs(dense).max())
            got = {'emulation': hr.worst_ratio(hr.cheb_emulate(kind, V, m, c, e), ref, E),
                   'degree m + 1': hr.worst_ratio(hr.cheb_emulate(kind, V, m + 1, c, e), ref, E)}
            if m >= 2:
                got['degree m - 1'] = hr.worst_ratio(hr.cheb_emulate(kind, V, m - 1, c, e), ref, E)
                got['-c/e for -2c/e'] = hr.worst_ratio(hr.cheb_emulate(kind, V, m, c, e, mistake='half_c'), ref, E)
            if m >= 3:
                got['y0 = V at degree 3'] = hr.worst_ratio(hr.cheb_emulate(kind, V, m, c, e, mistake='y0'), ref, E)
            print('kind %d %s cols=%d m=%d: %s; bound / result %.2g' % (kind, where, cols, m, ', '.join('%s %.3g' % kv for kv in got.items()), E.max() / np.abs(ref).max()))
            assert got.pop('emulation') <= 1.0
            assert all(v > WIDE for v in got.values()), got


@pytest.mark.parametrize('m,q', hr.F_LOCKED)
@pytest.mark.parametrize('kind', [0, 2])
def test_filter_with_locked_vectors_bound_holds_and_planted_mistakes_break_it(kind, m, q):
    c, e = hr.filter_interval(kind, 'inside')
    Q = hr.locked_block(kind)
    assert np.abs(Q.astype(np.float64).T @ Q.astype(np.float64) - np.eye(3)).max() < 1e-6
    for cols in hr.F_COLS:
        V = hr.filter_input(kind, cols)
        assert np.abs(Q.astype(np.float64).T @ V.astype(np.float64)).min() > 1e-3                  # V is not orthogonal to Q
        ref, E = hr.cheb_ref(kind, V, m, c, e, Q, q)
        got = {mis: hr.worst_ratio(hr.cheb_emulate(kind, V, m, c, e, Q, q, mistake=mis), ref, E) for mis in (None, 'skip', 'one_term', 'late')}
        print('kind %d m=%d q=%d cols=%d: emulation %.3g, projection skipped %.3g, one live term only %.3g, one degree late %.3g'
              % (kind, m, q, cols, got[None], got['skip'], got['one_term'], got['late']))
        assert got[None] <= 1.0
        assert got['skip'] > WIDE and got['one_term'] > WIDE
        if (m - 1) % q == 0 and m - q < 2:
            assert got['late'] > WIDE                                                              # the only projection falls behind degree m: (4, 3)
        else:
            assert got['late'] <= 1.0                                                              # commutes with the recurrence (module docstring)
        # what is left of Q in the block, against what the bound lets through
        left = np.abs(Q.astype(np.float64).T @ hr.cheb_emulate(kind, V, m, c, e, Q, q).astype(np.float64))
        assert np.all(left <= np.abs(Q.astype(np.float64).T @ ref) + np.abs(Q.astype(np.float64)).T @ E)


# ------------------------------------------------------------------------------------------------------------------ orth / orth_scaled
@pytest.mark.parametrize('scaled', [0, 1])
@pytest.mark.parametrize('case', hr.ORTH_CASES)
@pytest.mark.parametrize('b', hr.ORTH_B)
@pytest.mark.parametrize('n', hr.ORTH_N)
def test_orth_inputs_have_their_constructed_rank_far_from_every_threshold(n, b, case, scaled):
    Y, rank = hr.orth_input(n, b, case, scaled)
    G = Y.astype(np.float64).T @ Y.astype(np.float64)
    if scaled:                                                                                     # orth_scaled_pass: 1e-6 of the largest eigenvalue of the normalised Gram matrix
        d = np.where(np.diag(G) > 0, 1.0 / np.sqrt(np.where(np.diag(G) > 0, np.diag(G), 1.0)), 0.0)
        w = np.linalg.eigvalsh(G * d[:, None] * d[None, :])
        threshold = 1e-6 * w[-1]
    else:                                                                                          # orth_pass: tol lmax and abs_floor
        w = np.linalg.eigvalsh(G)
        threshold = max(hr.ORTH_ARGS[case][0] * w[-1], hr.ORTH_ARGS[case][1])
    w = np.sort(w)[::-1]
    assert np.all(w[:rank] >= 1e4 * threshold) and np.all(w[rank:] <= 1e-4 * threshold), (w[max(rank - 1, 0):rank + 1], threshold)
    Z = hr.orth_restated(Y, case, scaled)
    assert Z.dtype == np.float32 and Z.shape == (n, rank)
    assert hr.orth_defect(Z) < 2e-6
    assert hr.span_residual(Z, Y) <= hr.span_bound(Y, b)
    # a column that takes in 1e-3 of a direction from outside span(Y) is seen
    W = Z.copy(); W[:, 0] += np.float32(1e-3) * np.random.RandomState(0).randn(n).astype(np.float32)
    assert hr.span_residual(W, Y) > WIDE * hr.span_bound(Y, b)


# ------------------------------------------------------------------------------------------------------------------ spectrum estimates
@pytest.mark.parametrize('name', hr.EST_GRAPHS)
def test_spectrum_estimates_restated_in_fp64_lie_in_their_windows(name):
    g = hr.estimate_graph(name)
    assert g['n'] <= 1100
    smax, lo, hi = hr.hope_rho_window(g)
    rho, raw, steps = hr.hope_rho_emulate(g)
    print('%s: sigma_max %.6f, rho %.6f (%.4f sigma_max before the cap, %d steps), window [%.6f, %.6f]' % (name, smax, rho, raw / smax, steps, lo, hi))
    assert lo <= rho <= hi
    assert raw / 1.1 < smax                                                                        # an estimate from below: the margin is what lifts it into the window
    if name in hr.EST_UNDIRECTED:
        assert np.array_equal(g['dense'], g['dense'].T)
        s2, lo, hi = hr.lle_c_window(g)
        c, steps = hr.lle_c_emulate(g)
        print('%s: sigma_max(I - P)^2 %.6f, c %.6f = %.5f of it (%d steps), window [%.6f, %.6f]' % (name, s2, c, c / s2, steps, lo, hi))
        assert lo <= c <= hi
    assert hr.katz_terms(0.55) == 31 and hr.katz_terms(0.9499) == 359 and hr.katz_terms(0.99) == 400 and hr.katz_terms(1e-9) == 1
