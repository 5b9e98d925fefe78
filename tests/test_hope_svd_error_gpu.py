"""GPU: the `SVD error (low rank):` instrument (hope.hip svd_error_impl, through gemhip_hope_plan_svd_error_uv / _plan_svd_error) beyond one
128-column chunk of V, against the dense computation of hope.py:28-40 in fp64: S = (I - beta A)^-1 beta A, its SVD, ||u_k diag(s_k) v_k^T - S||_F.
U, V and sigma are the dense SVD rounded to fp32, so no solver takes part.  SBM-1024 (beta = 0.01) at k = 130, 160, 256: a second chunk of 2
columns, of 32 (cpad = 32) and a full one; a weighted directed graph of 400 nodes (beta ||A||_2 = 0.5) at k = 136, where a transposed operator
or exchanged U and V give another value (test_instrument_refs.py: +106 % and more).  The truncation part is a 32-probe estimate: its bar, 0.5 %
of the dense value, is six of the s.d. that test_instrument_refs.py measures for its fp64 restatement at these k (tests/README.md).  The U side
is exact and is tested as such: ~0 for the right U, 0.5 sigma_j (1e-3) for a column at half length -- in the second chunk and in the first."""
import ctypes as C

import numpy as np
import pytest

import instrument_refs as ir
from gem_amd import _hip
from gem_amd.graph import edge_arrays, to_csr

pytestmark = pytest.mark.gpu


class Operator(object):
    """One Katz plan on the device and its dense fp64 counterpart."""
    def __init__(self, n, src, dst, w, beta, A):
        self.n, self.beta = n, float(np.float32(beta))
        self.S = ir.katz_dense(A, self.beta)
        self.frob2 = float((self.S * self.S).sum())
        self.u, self.s, self.vt = np.linalg.svd(self.S)
        row_ptr, col, ww = to_csr(n, src, dst, w)
        self.plan = C.c_void_p()
        _hip.check(_hip.lib().gemhip_hope_plan_create(n, len(col), _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), _hip.ptr(ww, C.c_float), self.beta,
                                                      C.byref(self.plan)))

    def error(self, sig, U, V, seed=1):
        """(err, frob2, uside) of the _uv form, or (err, frob2, None) of the V-only form when U is None."""
        err = C.c_double(-1.0); frob2 = C.c_double(-1.0); us = C.c_double(-1.0)
        k = len(sig)
        L = _hip.lib()
        if U is None:
            _hip.check(L.gemhip_hope_plan_svd_error(self.plan, k, _hip.ptr(sig, C.c_float), _hip.ptr(V, C.c_float), 32, seed, C.byref(err), C.byref(frob2)))
            return err.value, frob2.value, None
        _hip.check(L.gemhip_hope_plan_svd_error_uv(self.plan, k, _hip.ptr(sig, C.c_float), _hip.ptr(U, C.c_float), _hip.ptr(V, C.c_float), 32, seed,
                                                   C.byref(err), C.byref(frob2), C.byref(us)))
        return err.value, frob2.value, us.value

    def close(self):
        _hip.check(_hip.lib().gemhip_hope_plan_destroy(self.plan))


@pytest.fixture(scope='module')
def sbm_operator(sbm1024):
    n, src, dst, w, order = edge_arrays(sbm1024)
    src, dst, w, A = ir.operator_arrays(n, src, dst, w, order)
    op = Operator(n, src, dst, w, 0.01, A)
    yield op
    op.close()


@pytest.fixture(scope='module')
def asym_operator():
    n, src, dst, w, beta, A = ir.asym_graph()
    op = Operator(n, src, dst, w, beta, A)
    yield op
    op.close()


def check_operator(op, what, k, j2, j1=5):
    """Every assertion of this file on one operator and one k; j2 is the column of the second chunk whose U is halved, j1 one of the first."""
    sig, U, V = ir.svd_inputs(op.u, op.s, op.vt, k)
    dense = ir.svd_error_dense(op.S, sig, U, V)
    err, frob2, uside = op.error(sig, U, V)
    print('SVD error %s k=%d: %.6g against the dense %.6g: %+.3f %% (bar %.1f %%); U side %.3g = %.2g of it (bar 2e-3); ||S||_F^2 %+.3f %%'
          % (what, k, err, dense, 100 * (err / dense - 1), 100 * ir.SVD_BAR, uside, uside / dense, 100 * (frob2 / op.frob2 - 1)))
    assert abs(err - dense) <= ir.SVD_BAR * dense
    assert 0.0 <= uside <= 2e-3 * dense
    assert abs(frob2 - op.frob2) <= ir.SVD_BAR * op.frob2                                     # frob2_out = err^2 + sum sigma^2 = ||S||_F^2
    assert frob2 == pytest.approx(err * err - uside * uside + float((sig.astype(np.float64) ** 2).sum()), rel=1e-12)
    # the V-only form is the truncation part of the _uv form: the same kernels on the same inputs and probes (fp32 atomics' order apart)
    err_v, frob2_v, _ = op.error(sig, None, V)
    assert frob2_v == pytest.approx(frob2, rel=1e-6) and err_v * err_v == pytest.approx(err * err - uside * uside, rel=1e-6)
    # one column of U at half length: the exact U side is 0.5 sigma_j wherever the column lives, and err follows the dense value of that factorisation
    for cols in ((j2,), (j1, j2)):
        assert all(0 <= j < k for j in cols) and 128 <= j2 and j1 < 128
        Ubad = U.copy(); Ubad[:, list(cols)] *= 0.5
        want_us = 0.5 * float(np.sqrt((sig[list(cols)].astype(np.float64) ** 2).sum()))
        dense_bad = ir.svd_error_dense(op.S, sig, Ubad, V)
        err_b, _, us_b = op.error(sig, Ubad, V)
        print('   U columns %s halved: U side %.6g against %.6g (%+.2e, bar 1e-3), err %.6g against the dense %.6g: %+.3f %%'
              % (cols, us_b, want_us, us_b / want_us - 1, err_b, dense_bad, 100 * (err_b / dense_bad - 1)))
        assert us_b == pytest.approx(want_us, rel=1e-3)
        assert abs(err_b - dense_bad) <= ir.SVD_BAR * dense_bad
    assert float(sig[j2]) ** 2 > 4e-3 * float((sig[[j1, j2]].astype(np.float64) ** 2).sum())   # (the second chunk's share of the pair is above the 1e-3 bar)
    return sig, U, V, err


@pytest.mark.parametrize('k,j2', ir.SVD_SBM_K)
def test_svd_error_beyond_one_chunk_on_sbm1024(sbm_operator, k, j2):
    check_operator(sbm_operator, 'SBM-1024', k, j2)


def test_svd_error_of_an_asymmetric_weighted_operator(asym_operator):
    op = asym_operator
    k = ir.SVD_ASYM_K
    sig, U, V, err = check_operator(op, 'asymmetric', k, 131)
    assert abs(ir.svd_error_dense(op.S.T, sig, U, V) - err) > 0.05 * err and abs(ir.svd_error_dense(op.S, sig, V, U) - err) > 0.05 * err
    # k above the rank: a zero singular value in the second chunk is skipped on both sides, not an error, and err is no smaller than with the column
    sig0 = sig.copy(); sig0[131] = 0.0
    err0, _, us0 = op.error(sig0, U, V)
    print('   sigma[131] = 0: err %.6g (with the column %.6g), U side %.3g' % (err0, err, us0))
    assert err0 >= err * (1 - 1e-3) and us0 <= 2e-3 * err
