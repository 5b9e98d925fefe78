"""CPU: the bounds of instrument_refs.py hold for a numpy emulation of each kernel's own arithmetic on every shape the GPU tests use, and a
planted mistake (an edge lost, the column k = d - 1 lost, a node's norm lost, the second chunk of V ignored) breaks them by a wide margin --
so the GPU tests (test_eval_ap_gpu.py, test_gf_objective_gpu.py, test_hope_svd_error_gpu.py) can fail."""
import numpy as np
import pytest

import oracle
import instrument_refs as ir
from gem_amd.evaluation import reconstruction as gr
from gem_amd.graph import edge_arrays

WIDE = 10.0            # "by a wide margin": a planted mistake is at least this many bounds away


# ------------------------------------------------------------------------------------------------------------------ sampled AP
@pytest.fixture(scope='module')
def ap_graph():
    return ir.ap_graph()


AP_ROWS = np.array([ir.AP_HUB, ir.AP_512, ir.AP_513, ir.AP_EMPTY, ir.AP_LOWER, ir.AP_TWICE, ir.AP_FAR, 0, 1, 100, 400, 698, 699])


@pytest.mark.parametrize('family', ['grid', 'random'])
@pytest.mark.parametrize('da,pad,kind,split', ir.AP_CASES)
def test_ap_bars_hold_for_the_kernels_summation_order_and_planted_mistakes_break_them(ap_graph, da, pad, kind, split, family):
    row_ptr, col, truth = ap_graph
    bar = ir.AP_GRID_BAR if family == 'grid' else ir.AP_RANDOM_BAR
    A, B = ir.ap_operands(da, pad, kind, split, family, seed=ir.ap_seed(da, kind))
    score, mag = ir.ap_dense_scores(A, B, da, kind)
    if family == 'random':
        assert ir.ap_reference_is_clear_of_ties(score, mag, da)
    else:
        assert all(len(np.unique(score[i])) < ir.AP_N - 1 for i in AP_ROWS if i != ir.AP_FAR), 'the grid family is there for its exact ties'
        if kind == 1:
            assert np.all(score[ir.AP_FAR] == 0.0) and np.all(score[:, ir.AP_FAR] == 0.0)
            off = score[~np.eye(ir.AP_N, dtype=bool) & (score > 0)]
            assert off.min() >= np.exp(-30.0)                                       # nothing else near exp's underflow
    for und in (True, False):
        ref = gr.average_precision_rows(score, truth, undirected=und)
        worst = 0.0; lost_column = 0.0; lost_edge = 0.0
        for i in AP_ROWS:
            row = col[row_ptr[i]:row_ptr[i + 1]]
            s = ir.ap_kernel_scores(A, B, da, kind, i)
            worst = max(worst, abs(ir.ap_by_counts(s, i, row, und) - ref[i]))
            lost_edge = max(lost_edge, abs(ir.ap_by_counts(s, i, row, und, drop_last_neighbour=True) - ref[i]))
            s1 = ir.ap_kernel_scores(A, B, da, kind, i, drop_last_column=True)
            lost_column = max(lost_column, abs(ir.ap_by_counts(s1, i, row, und) - ref[i]))
        print('AP %s kind %d da=%d und=%d: emulation %.3g, column lost %.3g, edge lost %.3g  (bar %.0e)' % (family, kind, da, und, worst, lost_column, lost_edge, bar))
        assert worst <= bar
        assert lost_edge > 1e-4 and lost_column > 1e-4                              # seven to eight orders above either bar
    if kind == 1 and family == 'grid':
        assert ref[ir.AP_FAR] == 0.0


# ------------------------------------------------------------------------------------------------------------------ GF objective
@pytest.mark.parametrize('name', ir.GF_CASES)
def test_gf_bound_holds_for_the_kernels_arithmetic_and_planted_mistakes_break_it(name):
    n, src, dst, w, d, X = ir.gf_case(name)
    m = len(src)
    f1, f2, b1, b2 = ir.gf_reference_and_bound(n, src, dst, w, d, X)
    o1, o2 = oracle.gf_objective(n, src, dst, np.ones(m, np.float32) if w is None else w, d, X)
    # the restatement the bound is built on == the oracle, up to fp64 summation order: far inside the bound also where the residuals cancel
    assert abs(o1 - f1) <= 1e-12 * f1 + 1e-3 * b1 and abs(o2 - f2) <= 1e-12 * f2
    for fma in (False, True):
        e1, e2 = ir.gf_emulate(n, src, dst, w, d, X, fma=fma)
        print('GF %s (n=%d m=%d d=%d, fma=%d): |f1 - ref| / bound = %.3g, |f2 - ref| / bound = %.3g' % (name, n, m, d, fma, abs(e1 - f1) / b1 if b1 else 0.0, abs(e2 - f2) / b2))
        assert abs(e1 - f1) <= b1 and abs(e2 - f2) <= b2
        if m == 0:
            assert e1 == 0.0 and b1 == 0.0
    if name == 'cancel':
        assert f1 < 1e-9 * m and b1 < 1e-9 * m                                              # the residuals are at rounding level: delta^2 is the bound
    # ---- planted mistakes
    if m and name != 'cancel':                             # (a lost edge of a cancelling list changes f1 by about bound / m: there the column shows)
        e1, _ = ir.gf_emulate(n, src, dst, w, d, X, drop_edge=m - 1)
        assert abs(e1 - f1) > WIDE * b1, ('last edge lost', abs(e1 - f1) / b1)
    if m:
        e1, e2 = ir.gf_emulate(n, src, dst, w, d, X, drop_last_column=True)
        assert abs(e1 - f1) > WIDE * b1, ('column d-1 lost, f1', abs(e1 - f1) / b1)
        assert abs(e2 - f2) > WIDE * b2, ('column d-1 lost, f2', abs(e2 - f2) / b2)
    _, e2 = ir.gf_emulate(n, src, dst, w, d, X, drop_node=n - 1)
    assert abs(e2 - f2) > WIDE * b2, ('last node lost', abs(e2 - f2) / b2)


def test_gf_grid_boundaries_are_where_the_cases_say():
    assert ir.GF_WAVES == 8192 and ir.GF_M == (1, ir.GF_WAVES - 1, ir.GF_WAVES, ir.GF_WAVES + 1)
    assert ir.gf_case('n8200')[0] > ir.GF_WAVES
    n, src, dst, w, d, X = ir.gf_case('d65')
    assert src[0] == dst[0] and dst[1] < src[1] and (src[1], dst[1]) == (src[2], dst[2])
    assert (w == 0).any() and (w < 0).any() and ir.gf_case('w_null')[3] is None


# ------------------------------------------------------------------------------------------------------------------ HOPE SVD error
def check_svd_estimate(B, S, ks, seed):
    """The spread of the 32-probe estimate over 200 seeds at each k (the statistic behind SVD_BAR), and the planted mistake."""
    n = S.shape[0]
    u, s, vt = np.linalg.svd(S)
    Z = np.random.RandomState(seed).randn(n, 200 * 32)
    out = {}
    for k in ks:
        sig, U, V = ir.svd_inputs(u, s, vt, k)
        dense = ir.svd_error_dense(S, sig, U, V)
        Vn = V.astype(np.float64) / np.sqrt(sig.astype(np.float64))
        est = ir.svd_trunc_estimates(B, S, Vn, Z)
        rel = est / dense - 1.0
        planted = ir.svd_trunc_estimates(B, S, Vn, Z[:, :32], bv_columns=128)[0] / dense - 1.0
        lost_u = ir.svd_uside_dense(S, sig, U, V, columns=128)
        print('SVD error k=%d: dense %.6g; 200 x 32 probes: bias %+.2e, s.d. %.4f %%, worst %.3f %% (bar %.1f %%); B V stopping at 128 columns: %+.2f %%'
              % (k, dense, rel.mean(), 100 * rel.std(), 100 * np.abs(rel).max(), 100 * ir.SVD_BAR, 100 * planted))
        assert rel.std() <= 1e-3, 'above 0.1 %: the bar for this k would be six times this'
        assert np.abs(rel).max() <= ir.SVD_BAR and abs(rel.mean()) <= 5e-4
        assert lost_u <= 2e-3 * dense                          # the exact U side of a correct factorisation
        out[k] = (dense, planted, sig, U, V)
    return out


def test_svd_error_bar_on_sbm1024_and_a_second_chunk_that_is_ignored(sbm1024):
    n, src, dst, w, order = edge_arrays(sbm1024)
    A = ir.operator_arrays(n, src, dst, w, order)[3]
    B = np.float64(np.float32(0.01)) * A
    S = ir.katz_dense(A, np.float64(np.float32(0.01)))
    res = check_svd_estimate(B, S, [k for k, _ in ir.SVD_SBM_K], seed=3)
    for k, j in ir.SVD_SBM_K:
        dense, planted, sig, U, V = res[k]
        assert 128 <= j < k
        # the truncation estimate sees an ignored second chunk once the chunk is wide enough; its two columns at k = 130 carry 2 of ~900 parts of
        # err^2, under any statistical bar -- there (and at every k) the EXACT U side shows it: the halved column gives 0.5 sigma_j, a loop that
        # stops at 128 gives 0
        if k >= 160:
            assert planted > WIDE / 2 * ir.SVD_BAR, (k, planted)
        Ubad = U.copy(); Ubad[:, j] *= 0.5
        whole = ir.svd_uside_dense(S, sig, Ubad, V); first = ir.svd_uside_dense(S, sig, Ubad, V, columns=128)
        assert whole == pytest.approx(0.5 * float(sig[j]), rel=1e-3) and first < 1e-2 * whole


def test_svd_error_bar_on_the_asymmetric_graph_and_a_transposed_operator():
    n, src, dst, w, beta, A = ir.asym_graph()
    assert 380 <= n <= 420 and w.min() > 0 and w.max() < 2 and not np.array_equal(A, A.T)
    assert np.float32(beta) * np.linalg.norm(A, 2) == pytest.approx(0.5, rel=1e-3)
    B = beta * A
    S = ir.katz_dense(A, beta)
    k = ir.SVD_ASYM_K
    dense, planted, sig, U, V = check_svd_estimate(B, S, [k], seed=4)[k]
    assert planted > WIDE / 2 * ir.SVD_BAR
    Vn = V.astype(np.float64) / np.sqrt(sig.astype(np.float64))
    Z = np.random.RandomState(5).randn(n, 32)
    transposed = ir.svd_trunc_estimates(B.T, S.T, Vn, Z)[0]
    swapped = ir.svd_error_dense(S, sig, V, U)
    print('asymmetric graph k=%d: dense %.6g, with A^T %.6g (%+.1f %%), with U and V exchanged %.6g' % (k, dense, transposed, 100 * (transposed / dense - 1), swapped))
    assert abs(transposed - dense) > 0.05 * dense and abs(swapped - dense) > 0.05 * dense
    assert abs(ir.svd_error_dense(S.T, sig, U, V) - dense) > 0.05 * dense
