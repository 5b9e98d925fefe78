"""GPU: gemhip_gf_objective (gf_objective_kernel: f1 = sum_e (w - X_i.X_j)^2 over ALL edges, f2 = ||X||_F^2, gf.cpp:94-113) against the fp64
oracle with the DERIVED bound of instrument_refs.gf_reference_and_bound, on every shape at which the kernel takes another path: d below, at and
above a wavefront's 64 lanes and no multiple of it, one to 8193 edges around the 8192 wavefronts of the fixed grid, no edge, one node, more
nodes than wavefronts, w == NULL, zero and negative weights, self-loops, dst < src, a repeated edge, and residuals that cancel (there the
bound is its delta^2 term and a relative tolerance would mean nothing).  test_instrument_refs.py holds the bound against a numpy emulation of
the kernel's arithmetic and shows that a lost edge, column or node breaks it tenfold."""
import ctypes as C

import numpy as np
import pytest

import oracle
import instrument_refs as ir
from gem_amd import _hip

pytestmark = pytest.mark.gpu


def hip_objective(n, src, dst, w, d, X):
    out = (C.c_double * 2)(-1.0, -1.0)
    m = len(src)
    _hip.check(_hip.lib().gemhip_gf_objective(n, m, _hip.ptr(src if m else None, C.c_int32), _hip.ptr(dst if m else None, C.c_int32),
                                              _hip.ptr(w if m else None, C.c_float), d, _hip.ptr(X, C.c_float), out))
    return out[0], out[1]


@pytest.mark.parametrize('name', ir.GF_CASES)
def test_objective_within_the_derived_bound(name):
    n, src, dst, w, d, X = ir.gf_case(name)
    m = len(src)
    f1, f2, b1, b2 = ir.gf_reference_and_bound(n, src, dst, w, d, X)
    o1, o2 = oracle.gf_objective(n, src, dst, np.ones(m, np.float32) if w is None else w, d, X)
    assert abs(o1 - f1) <= 1e-12 * f1 + 1e-3 * b1 and abs(o2 - f2) <= 1e-12 * f2           # the bound's own f1, f2 are the oracle's
    g1, g2 = hip_objective(n, src, dst, w, d, X)
    print('GF objective %s (n=%d m=%d d=%d): f1 %.9g, |f1 - oracle| / bound = %.3g; f2 %.9g, |f2 - oracle| / bound = %.3g'
          % (name, n, m, d, g1, abs(g1 - o1) / b1 if b1 else 0.0, g2, abs(g2 - o2) / b2))
    assert abs(g1 - o1) <= b1 and abs(g2 - o2) <= b2
    if m == 0:
        assert g1 == 0.0 and b1 == 0.0
    assert hip_objective(n, src, dst, w, d, X)[1] == pytest.approx(g2, rel=n * 2.0 ** -50)   # (the atomics' order is free, nothing else)
