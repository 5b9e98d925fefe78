"""GPU kernel-level parity of HOPE's device building blocks UNDER THE SOLVERS' CALLING CONVENTIONS (the gemhip_test_hope_* hooks of
include/gem_hip.h: each uploads host blocks, calls the host function the solvers call -- spmm, gram, gram2, tsgemm, ritz_rotate, colmax,
project_out, apply_sym_op, lincomb, randn -- and copies the result back).  test_hope_kernels_gpu.py reaches three of them with compact
blocks, the plain epilogue and distinct buffers; here: every SpMM instantiation, the three-term epilogue, leading dimensions above the
logical width, column offsets, blocks that alias (Wadd = X, W2 = Y, Out = Src), and the blocks no other test calls.

References are numpy fp64 computations of the same operation on the same fp32 inputs.  Tolerances are derived, not measured: a length-L fp32
dot product or sum, taken in any order and with or without fused multiply-adds, is within (L + c) * 2^-23 * sum_k |a_k| |b_k| of the exact
value, c (<= 4) counting the epilogue's terms; sum |a| |b| comes from the reference on the absolute values and the comparison is elementwise.
Every block with ld above its logical width carries a sentinel in the padding, which must survive the call."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from gem_amd import _hip

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
SENT = np.float32(-12345.0)                       # the padding's sentinel: no computed value comes near it


def f32(x):
    return float(np.float32(x))


def fp(a):
    return _hip.ptr(a, C.c_float)


def dp(a):
    return _hip.ptr(a, C.c_double)


def padded(A, ld, off=0):
    """A (n x m) as columns [off, off + m) of an n x ld block whose other columns hold the sentinel."""
    n, m = A.shape
    P = np.full((n, ld), SENT, np.float32)
    P[:, off:off + m] = A
    return P


def assert_padding(P, off, m):
    """Nothing outside columns [off, off + m) was written."""
    mask = np.ones(P.shape[1], bool); mask[off:off + m] = False
    assert np.all(P[:, mask] == SENT), 'a padding column was overwritten'


# ------------------------------------------------------------------------------------------------------------------ SpMM
CRAFTED_DEGREES = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]       # around the 16- and 64-neighbour batches of the two kernels


def make_graph(n, seed):
    """CSR with the crafted degrees at the first rows, random degrees after them, a LAST row of degree 0, signed fp32 weights.
    n = 203 is no multiple of 16 or 4: the last 16-lane group and the last wavefront block are partial.  n = 1: one self loop."""
    rng = np.random.RandomState(seed)
    if n == 1:
        deg = np.array([1])
    else:
        deg = np.concatenate([CRAFTED_DEGREES, rng.randint(0, 40, n - len(CRAFTED_DEGREES) - 1), [0]])
    rp = np.zeros(n + 1, np.int64); rp[1:] = np.cumsum(deg)
    ci = np.concatenate([rng.choice(n, d, replace=False) for d in deg] + [np.zeros(0, np.int64)]).astype(np.int32)
    va = ((rng.rand(len(ci)) + 0.1) * rng.choice([-1.0, 1.0], len(ci))).astype(np.float32)
    A = sp.csr_matrix((va.astype(np.float64), ci.copy(), rp.copy()), shape=(n, n))       # (copies: scipy sorts a row's columns in place; the kernels get them unsorted)
    return dict(n=n, rp=rp, ci=ci, va=va, A=A, absA=abs(A), deg=deg.astype(np.float64))


_graphs = {}


def graph(n):
    if n not in _graphs:
        _graphs[n] = make_graph(n, 7 + n)
    return _graphs[n]


def expected_instantiation(b, variant):
    """hope_ops.hip spmm(): the 16-lane kernel up to 128 columns -- <ceil(b / 16), U> with U = 8 up to 48 columns and 4 beyond, 6 sixteenths only with
    U <= 4, 7 and 8 sixteenths as <8, 2> -- else one row per wavefront, <CPL> in {1, 2, 4, 8} (reported with U = 0)."""
    if variant == 1 or b > 128:
        cpl = (b + 63) // 64
        return (1 if cpl <= 1 else 2 if cpl <= 2 else 4 if cpl <= 4 else 8, 0)
    c16 = (b + 15) // 16
    u = variant if variant else (8 if c16 <= 3 else 4)
    return (c16, u) if c16 <= 5 else (6, min(u, 4)) if c16 == 6 else (8, 2)


def run_spmm(g, variant, alpha, b, X, ldx, Y, ldy, wa=1.0, W=None, ldw=0, wb=0.0, W2=None, ldw2=0, w_is_x=0, w2_is_y=0):
    launched = np.zeros(2, np.int32)
    _hip.check(_hip.lib().gemhip_test_hope_spmm(g['n'], len(g['ci']), _hip.ptr(g['rp'], C.c_int64), _hip.ptr(g['ci'], C.c_int32), fp(g['va']), variant,
                                                alpha, b, fp(X), ldx, wa, fp(W), ldw, wb, fp(W2), ldw2, w_is_x, w2_is_y, fp(Y), ldy,
                                                _hip.ptr(launched, C.c_int32)))
    assert tuple(launched) == expected_instantiation(b, variant), 'b = %d, variant %d launched %s' % (b, variant, tuple(launched))
    return Y


def spmm_ref(g, alpha, X, wa=0.0, W=None, wb=0.0, W2=None):
    """(reference, elementwise bound) of alpha A X + wa W + wb W2: L = the row's degree, c = 4."""
    X = X.astype(np.float64)
    ref = alpha * (g['A'] @ X); mag = abs(alpha) * (g['absA'] @ np.abs(X))
    if W is not None:
        ref = ref + wa * W.astype(np.float64); mag = mag + abs(wa) * np.abs(W).astype(np.float64)
    if W2 is not None:
        ref = ref + wb * W2.astype(np.float64); mag = mag + abs(wb) * np.abs(W2).astype(np.float64)
    return ref, (g['deg'][:, None] + 4) * U * mag


def spmm_forms(g, variant, b):
    """Every calling convention of the solvers for one (graph, kernel variant, width)."""
    n = g['n']
    rng = np.random.RandomState(1000 * b + variant)
    X, W, W2 = (rng.randn(n, b).astype(np.float32) for _ in range(3))
    alpha, wa, wb = f32(0.37), f32(-1.3), f32(0.6)
    ld = b + 3

    def check(Yp, off, ref, bound, what):
        err = np.abs(Yp[:, off:off + b].astype(np.float64) - ref)
        assert np.all(err <= bound), '%s: error %.3g over the bound at %s' % (what, (err - bound).max(), np.unravel_index(np.argmax(err - bound), err.shape))
        assert_padding(Yp, off, b)

    for ldc in (b, ld):                                                           # compact blocks, then ld = b + 3 on all four arrays
        Xp, Wp, W2p = padded(X, ldc), padded(W, ldc), padded(W2, ldc)
        blank = lambda: np.full((n, ldc), SENT, np.float32)
        tag = 'b=%d variant=%d ld=%d ' % (b, variant, ldc)
        check(run_spmm(g, variant, alpha, b, Xp, ldc, blank(), ldc), 0, *spmm_ref(g, alpha, X), tag + 'plain')
        check(run_spmm(g, variant, alpha, b, Xp, ldc, blank(), ldc, 1.0, Wp, ldc), 0, *spmm_ref(g, alpha, X, 1.0, W), tag + '+Wadd')
        check(run_spmm(g, variant, alpha, b, Xp, ldc, blank(), ldc, wa, Wp, ldc, wb, W2p, ldc), 0, *spmm_ref(g, alpha, X, wa, W, wb, W2), tag + 'three terms')
        check(run_spmm(g, variant, alpha, b, Xp, ldc, blank(), ldc, wa, Wp, ldc), 0, *spmm_ref(g, alpha, X, wa, W), tag + 'wa != 1, no W2')
        # Wadd IS X: (I + M) X and X - P X
        check(run_spmm(g, variant, -1.0, b, Xp, ldc, blank(), ldc, 1.0, None, 0, 0.0, None, 0, 1, 0), 0, *spmm_ref(g, -1.0, X, 1.0, X), tag + 'Wadd = X')
        check(run_spmm(g, variant, alpha, b, Xp, ldc, blank(), ldc, wa, None, 0, wb, W2p, ldc, 1, 0), 0, *spmm_ref(g, alpha, X, wa, X, wb, W2), tag + 'Wadd = X, three terms')
        # W2 IS Y: apply_sym_op kind 2 (Y holds W2 on entry; its padding holds the sentinel)
        check(run_spmm(g, variant, alpha, b, Xp, ldc, W2p.copy(), ldc, wa, Wp, ldc, 1.0, None, 0, 0, 1), 0, *spmm_ref(g, alpha, X, wa, W, 1.0, W2), tag + 'W2 = Y')
        check(run_spmm(g, variant, -alpha, b, Xp, ldc, W2p.copy(), ldc, alpha, None, 0, 1.0, None, 0, 1, 1), 0, *spmm_ref(g, -alpha, X, alpha, X, 1.0, W2),
              tag + 'Wadd = X and W2 = Y')
    if b == 1:                                                                    # the power iteration's blocks: x = column 0 of [x | z], y of ld 1, z = column 1
        X2 = padded(X, 2)
        y = run_spmm(g, variant, 1.0, 1, X2, 2, np.full((n, 1), SENT, np.float32), 1)
        check(y, 0, *spmm_ref(g, 1.0, X), 'ldx = 2, ldy = 1')
        Z2 = run_spmm(g, variant, 1.0, 1, y, 1, np.ascontiguousarray(X2[:, ::-1]), 2)          # into column 0 of a block whose column 1 is data
        check(padded(Z2[:, :1], 1), 0, *spmm_ref(g, 1.0, y), 'ldx = 1, ldy = 2')
        assert np.array_equal(Z2[:, 1], X[:, 0]), 'the neighbouring column of an ld = 2 block was overwritten'


SPMM16_WIDTHS = [1, 16, 17, 33, 48, 49, 64, 65, 81, 96, 97, 113, 128]


def u_variants(b):
    """Forced U values that have an instantiation of their own at this width (hope_ops.hip spmm(): U = 8 up to 80 columns, U = 4 up to 96)."""
    c16 = (b + 15) // 16
    return [2, 4, 8] if c16 <= 5 else [2, 4] if c16 <= 6 else [2]


SPMM_CASES = [(b, v) for b in SPMM16_WIDTHS for v in [0] + u_variants(b)] + [(b, 1) for b in (1, 64, 65, 128, 129, 257, 512)] + [(129, 0), (512, 0)]


@pytest.mark.parametrize('b,variant', SPMM_CASES)
def test_spmm_every_instantiation_and_calling_convention(b, variant):
    for n in (203, 1):
        spmm_forms(graph(n), variant, b)


@pytest.mark.parametrize('b', SPMM16_WIDTHS)
def test_spmm_variants_are_bit_identical(b):
    """Every U of the 16-lane kernel forms the same products and adds them in the same (edge) order: with the plain epilogue the forced
    variants and the default dispatch agree bit for bit.  The one-row-per-wavefront kernel adds in the same order too, but its multiply-adds
    are fused where the 16-lane kernel's are a (packed) multiply and an add: the two agree to rounding -- each within the derived bound of the
    fp64 reference, hence within twice the bound of one another -- not bit for bit."""
    g = graph(203)
    rng = np.random.RandomState(b)
    X = rng.randn(203, b).astype(np.float32); W = rng.randn(203, b).astype(np.float32)
    alpha = f32(0.37)
    for Wadd in (None, W):
        outs = {v: run_spmm(g, v, alpha, b, X, b, np.full((203, b), SENT, np.float32), b, 1.0, Wadd, b) for v in [0, 1] + u_variants(b)}
        for v in u_variants(b):
            assert np.array_equal(outs[v].view(np.uint32), outs[0].view(np.uint32)), 'U = %d differs from the default dispatch at b = %d' % (v, b)
        _, bound = spmm_ref(g, alpha, X, 1.0, Wadd)
        assert np.all(np.abs(outs[1].astype(np.float64) - outs[0].astype(np.float64)) <= 2 * bound)


def test_spmm_knobs_are_read_at_every_call(monkeypatch):
    """GEMHIP_HOPE_SPMM16 and GEMHIP_HOPE_SPMM16_U are read when a hook (a plan set-up, a solve) starts, not frozen at the first SpMM of the
    process: three production-dispatch calls (variant 0) in one process, under SPMM16=0, under SPMM16=1 with SPMM16_U=2, and with both unset,
    launch <1> of the one-row kernel, <1, 2> and <1, 8> of the 16-lane kernel at b = 8.

    The two 16-lane outputs are equal bit for bit, padding sentinel included.  The one-row kernel's is not held to that: both kernels add a row's
    neighbours in CSR order, but the one-row kernel's multiply-adds are fused and the 16-lane kernel's are not (hope_ops.hip says so at the
    kernel, test_spmm_variants_are_bit_identical above holds them to rounding only), so the outputs are not bit-equal before this change
    either.  All three are therefore compared with the fp64 reference under that test's derived bound, elementwise, and their padding must
    hold the sentinel."""
    n, b, ld = 200, 8, 11
    g = make_graph(n, 207)
    rng = np.random.RandomState(8)
    X = rng.randn(n, b).astype(np.float32)
    alpha = f32(0.37)
    ref, bound = spmm_ref(g, alpha, X)

    def call(env):
        for name in ('GEMHIP_HOPE_SPMM16', 'GEMHIP_HOPE_SPMM16_U'):
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        Y, launched = np.full((n, ld), SENT, np.float32), np.zeros(2, np.int32)
        _hip.check(_hip.lib().gemhip_test_hope_spmm(n, len(g['ci']), _hip.ptr(g['rp'], C.c_int64), _hip.ptr(g['ci'], C.c_int32), fp(g['va']), 0, alpha, b,
                                                    fp(padded(X, ld)), ld, 1.0, None, 0, 0.0, None, 0, 0, 0, fp(Y), ld, _hip.ptr(launched, C.c_int32)))
        return Y, tuple(launched)

    one_row, l0 = call({'GEMHIP_HOPE_SPMM16': '0'})
    u2, l1 = call({'GEMHIP_HOPE_SPMM16': '1', 'GEMHIP_HOPE_SPMM16_U': '2'})
    auto, l2 = call({})
    assert (l0, l1, l2) == ((1, 0), (1, 2), (1, 8))
    assert np.array_equal(u2.view(np.uint32), auto.view(np.uint32)), 'U = 2 and the default U differ'
    for name, Y in (('SPMM16=0', one_row), ('SPMM16_U=2', u2), ('unset', auto)):
        err = np.abs(Y[:, :b].astype(np.float64) - ref)
        print('%s: max error / bound = %.3g' % (name, (err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), name
        assert_padding(Y, 0, b)
    print('one-row against 16-lane: %d of %d values differ in their bits' % (np.count_nonzero(one_row.view(np.uint32) != auto.view(np.uint32)), one_row.size))


# ------------------------------------------------------------------------------------------------------------------ Ritz rotation
RITZ_SHAPES = [(1, 1, 1), (33, 7, 1), (100, 8, 31), (515, 9, 33), (1000, 40, 32), (4097, 448, 96)]


@pytest.mark.parametrize('regime', ['random', 'near_converged'])
@pytest.mark.parametrize('n,m,b2', RITZ_SHAPES)
def test_ritz_rotation_and_residual_norms(n, m, b2, regime):
    rng = np.random.RandomState(n + m + b2)
    if regime == 'random':
        V = rng.randn(n, m); B = rng.randn(n, m); Cm = rng.randn(m, b2); theta = rng.randn(b2)
    else:
        # B = V S + 1e-3 noise with orthonormal V: (theta, C) = eigenpairs of sym(V^T B), so B C and theta V C cancel to ~1e-3 of their size
        V, _ = np.linalg.qr(rng.randn(n, m))
        S = rng.randn(m, m); S = (S + S.T) / 2
        B = V @ S + 1e-3 * rng.randn(n, m) / np.sqrt(n)
        Hm = V.T @ B
        w, Z = np.linalg.eigh((Hm + Hm.T) / 2)
        pick = np.arange(b2) % m                                              # b2 may exceed m: the pairs repeat
        Cm = Z[:, pick]; theta = w[pick]
    V = V.astype(np.float32); B = B.astype(np.float32)
    ldv, off, ldo = m + 5, 3, b2 + 2
    Vp, Bp = padded(V, ldv, off), padded(B, ldv, off)
    Out = np.full((n, ldo), SENT, np.float32); res2 = np.full(b2, np.nan)
    Cm = np.ascontiguousarray(Cm, dtype=np.float64); theta = np.ascontiguousarray(theta, dtype=np.float64)
    _hip.check(_hip.lib().gemhip_test_hope_ritz(n, fp(Vp), ldv, off, fp(Bp), ldv, off, m, dp(Cm), dp(theta), b2, fp(Out), ldo, dp(res2)))
    C32 = Cm.astype(np.float32).astype(np.float64); th = theta.astype(np.float32).astype(np.float64)          # what the kernel is given
    V64, B64 = V.astype(np.float64), B.astype(np.float64)
    vc = V64 @ C32; avc = np.abs(V64) @ np.abs(C32)
    assert np.all(np.abs(Out[:, :b2] - vc) <= (m + 3) * U * avc)
    assert_padding(Out, 0, b2)
    r = B64 @ C32 - th * vc
    delta = (m + 3) * U * (np.abs(B64) @ np.abs(C32) + np.abs(th) * avc)          # elementwise bound of the kernel's r
    rn = np.linalg.norm(r, axis=0)
    assert np.all(res2 >= 0)
    assert np.all(np.abs(np.sqrt(res2) - rn) <= np.linalg.norm(delta, axis=0) + 1e-5 * rn)     # 1e-5: the fp32 partial sums of squares
    if regime == 'near_converged' and n > 1:
        assert rn.max() < 0.1 * np.linalg.norm(B64 @ C32, axis=0).max()            # the regime is what it says: the terms do cancel


# ------------------------------------------------------------------------------------------------------------------ column arg-max
def colmax_chunks(n):
    nchunks = min(512, (n + 63) // 64)
    return (n + nchunks - 1) // nchunks                                            # rows per chunk of the two-pass kernel


@pytest.mark.parametrize('mc', [1, 63, 64, 65, 96])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000, 40000])
def test_colmax_largest_magnitude_first_row_on_ties(n, mc):
    """Values on a coarse grid: exact magnitude ties with opposite signs in every column; the expected value is numpy's first occurrence.
    Then the maximum is planted at row 0, at the last row and on both sides of a chunk boundary, with a later row of the opposite sign."""
    rng = np.random.RandomState(n * 100 + mc)
    ld = mc + 2
    base = (np.round(rng.randn(n, mc) * 2) / 2).astype(np.float32)
    rpc = colmax_chunks(n)
    signs = np.where(np.arange(mc) % 2 == 0, 1.0, -1.0).astype(np.float32)
    cases = [base]
    for row in sorted({0, n - 1, rpc - 1, min(rpc, n - 1), n // 2}):
        X = base.copy(); X[row] = 9.0 * signs
        later = rng.randint(row, n)                                               # (row itself: no second candidate)
        if later > row:
            X[later] = -9.0 * signs
        cases.append(X)
    for X in cases:
        want = X[np.argmax(np.abs(X), axis=0), np.arange(mc)]
        Xp = padded(X, ld)
        for variant in (1, 2, 0):
            val = np.full(mc, np.nan, np.float32)
            _hip.check(_hip.lib().gemhip_test_hope_colmax(n, fp(Xp), ld, mc, variant, fp(val)))
            assert np.array_equal(val, want), 'variant %d: columns %s' % (variant, np.nonzero(val != want)[0][:8])


# ------------------------------------------------------------------------------------------------------------------ Gram, Gf, gram2
GRAM_SHAPES = [(7, 3, 2), (4097, 33, 70), (1000, 31, 32)]


def run_gram(n, Xp, ldx, xoff, m1, Yp, ldy, yoff, m2, want_gf=False):
    G = np.full((m1, m2), np.nan); Gf = np.full((m1, m2), np.nan, np.float32) if want_gf else None
    _hip.check(_hip.lib().gemhip_test_hope_gram(n, fp(Xp), ldx, xoff, m1, fp(Yp), ldy, yoff, m2, dp(G), fp(Gf)))
    return G, Gf


def gram_inputs(n, m1, m2):
    rng = np.random.RandomState(n)
    X = rng.randn(n, m1).astype(np.float32); Y = (rng.randn(n, m2) + np.arange(m2) * 0.01).astype(np.float32)   # asymmetric on purpose
    return X, Y


def check_gram(G, X, Y):
    n = X.shape[0]
    ref = X.astype(np.float64).T @ Y.astype(np.float64)
    assert np.all(np.abs(G - ref) <= (n + 4) * U * (np.abs(X).astype(np.float64).T @ np.abs(Y).astype(np.float64)))
    assert np.abs(G - ref).max() <= 3e-6 * np.sqrt(n) * 4 + 1e-5 * np.abs(ref).max()                             # test_hope_kernels_gpu.py's assertion


@pytest.mark.parametrize('n,m1,m2', GRAM_SHAPES)
def test_gram_with_strides_offsets_and_fp32_rounding(n, m1, m2):
    X, Y = gram_inputs(n, m1, m2)
    Xp, Yp = padded(X, m1 + 4, 1), padded(Y, m2 + 4, 3)
    G, Gf = run_gram(n, Xp, m1 + 4, 1, m1, Yp, m2 + 4, 3, m2, want_gf=True)
    check_gram(G, X, Y)
    assert np.array_equal(Gf, G.astype(np.float32))
    G0, _ = run_gram(n, X, m1, 0, m1, Y, m2, 0, m2)                                # compact blocks through gram(): the strides change no bit
    assert np.array_equal(G0, G)
    legacy = np.empty((m1, m2))
    _hip.check(_hip.lib().gemhip_hope_gram(n, m1, m2, fp(X), fp(Y), dp(legacy)))
    assert np.array_equal(legacy, G)
    # two column blocks of ONE device block (gram(Va, Va) / the [x | z] block of the power iterations)
    Z = np.concatenate([X, Y], axis=1); Zp = padded(Z, m1 + m2 + 4, 2)
    Gs = np.full((m1, m2), np.nan)
    _hip.check(_hip.lib().gemhip_test_hope_gram(n, fp(Zp), m1 + m2 + 4, 2, m1, None, 0, 2 + m1, m2, dp(Gs), None))
    assert np.array_equal(Gs, G)


@pytest.mark.parametrize('n,m1,m2', GRAM_SHAPES)
def test_gram2_equals_two_single_grams(n, m1, m2):
    """Two products of different shapes through the shared slab scratch in stream order, each into its own fp64 block."""
    X, Y = gram_inputs(n, m1, m2)
    ldx, ldy = m1 + 4, m2 + 4
    Xp, Yp = padded(X, ldx, 1), padded(Y, ldy, 3)
    Gxy, _ = run_gram(n, Xp, ldx, 1, m1, Yp, ldy, 3, m2)
    Gyy, _ = run_gram(n, Yp, ldy, 3, m2, Yp, ldy, 3, m2)
    check_gram(Gyy, Y, Y)
    for first in ('xy', 'yy'):
        Ga = np.full((m1, m2) if first == 'xy' else (m2, m2), np.nan); Gb = np.full((m2, m2) if first == 'xy' else (m1, m2), np.nan)
        a = (fp(Xp), ldx, 1, m1, fp(Yp), ldy, 3, m2); b = (fp(Yp), ldy, 3, m2, fp(Yp), ldy, 3, m2)
        if first == 'yy':
            a, b = b, a
        _hip.check(_hip.lib().gemhip_test_hope_gram2(n, *a, dp(Ga), *b, dp(Gb)))
        assert np.array_equal(Ga, Gxy if first == 'xy' else Gyy) and np.array_equal(Gb, Gyy if first == 'xy' else Gxy)


# ------------------------------------------------------------------------------------------------------------------ tall-skinny GEMM
@pytest.mark.parametrize('n,m,b2', RITZ_SHAPES + [(7, 3, 2), (4097, 33, 70), (1000, 31, 32)])
def test_tsgemm_with_strides_offset_and_in_place(n, m, b2):
    rng = np.random.RandomState(m + b2)
    X = rng.randn(n, m).astype(np.float32); Cm = rng.randn(m, b2); S = rng.randn(n, b2).astype(np.float32)
    alpha = -0.5
    ldx, xoff, ldo, lds = m + 5, 3, b2 + 2, b2 + 1
    Xp = padded(X, ldx, xoff)
    prod = X.astype(np.float64) @ Cm.astype(np.float32).astype(np.float64)
    aprod = np.abs(X).astype(np.float64) @ np.abs(Cm.astype(np.float32)).astype(np.float64)

    def run(src, lds_, in_place, Out):
        _hip.check(_hip.lib().gemhip_test_hope_tsgemm(n, fp(Xp), ldx, xoff, m, dp(Cm), b2, alpha, fp(src), lds_, in_place, fp(Out), ldo))
        return Out
    outs = []
    for src in (None, S):
        ref = (0 if src is None else src.astype(np.float64)) + alpha * prod
        bound = (m + 3) * U * ((0 if src is None else np.abs(src).astype(np.float64)) + abs(alpha) * aprod)
        O = run(None if src is None else padded(src, lds), lds, 0, np.full((n, ldo), SENT, np.float32))
        assert np.all(np.abs(O[:, :b2] - ref) <= bound)
        assert np.abs(O[:, :b2] - ref).max() <= 1e-5 * np.sqrt(m) * max(np.abs(ref).max(), 1.0)                # test_hope_kernels_gpu.py's assertion
        assert_padding(O, 0, b2)
        outs.append(O)
    Oi = run(None, 0, 1, padded(S, ldo))                                           # Out == Src: the device block is read and overwritten
    assert np.array_equal(Oi, outs[1])
    legacy = np.empty((n, b2), np.float32)
    _hip.check(_hip.lib().gemhip_hope_tsgemm(n, m, b2, fp(X), dp(Cm), alpha, fp(S), fp(legacy)))
    assert np.array_equal(legacy, outs[1][:, :b2])                                 # strides and offset change no bit


# ------------------------------------------------------------------------------------------------------------------ project_out
@pytest.mark.parametrize('cols', [1, 33])
@pytest.mark.parametrize('m', [1, 9, 64])
@pytest.mark.parametrize('n', [33, 1000])
def test_project_out_on_device(n, m, cols):
    rng = np.random.RandomState(n + 10 * m + cols)
    Q, _ = np.linalg.qr(rng.randn(n, min(m, n)))                                   # orthonormal V (n = 33 < m = 64: the first 33 columns are)
    V = np.zeros((n, m)); V[:, :Q.shape[1]] = Q
    V = V.astype(np.float32); W = rng.randn(n, cols).astype(np.float32)
    ldv, ldw = m + 3, cols + 2
    Wp = padded(W, ldw)
    _hip.check(_hip.lib().gemhip_test_hope_project_out(n, fp(padded(V, ldv)), ldv, m, fp(Wp), ldw, cols, -1))
    assert_padding(Wp, 0, cols)
    Wo = Wp[:, :cols]
    # (1) the same arithmetic as gram() + fp32 rounding + tsgemm() through the existing exports, bit for bit
    G = np.empty((m, cols)); step = np.empty((n, cols), np.float32)
    _hip.check(_hip.lib().gemhip_hope_gram(n, m, cols, fp(V), fp(W), dp(G)))
    _hip.check(_hip.lib().gemhip_hope_tsgemm(n, m, cols, fp(V), dp(G), -1.0, fp(W), fp(step)))
    assert np.array_equal(Wo, step)
    # (2) as in the solvers: W = a column block of V's own device block
    ldb, woff = m + cols + 3, m + 1
    Bp = padded(np.concatenate([V, np.full((n, 1), SENT, np.float32), W], axis=1), ldb)
    _hip.check(_hip.lib().gemhip_test_hope_project_out(n, fp(Bp), ldb, m, fp(Bp), ldb, cols, woff))
    assert np.array_equal(Bp[:, woff:woff + cols], step) and np.array_equal(Bp[:, :m], V)
    assert np.all(Bp[:, m] == SENT) and np.all(Bp[:, woff + cols:] == SENT)
    # (3) the derived bound against W - V (V^T W) in fp64.  G~ = fl32(V^T W) is within e1 = (n + 1) u |V|^T |W| of V^T W (the + 1: its rounding
    # to fp32); the GEMM adds (m + 2) u (|W| + |V| |G~|) and carries e1 through |V|.
    V64, W64 = V.astype(np.float64), W.astype(np.float64)
    aG = np.abs(V64).T @ np.abs(W64)
    e1 = (n + 1) * U * aG
    ref = W64 - V64 @ (V64.T @ W64)
    assert np.all(np.abs(Wo - ref) <= np.abs(V64) @ e1 + (m + 2) * U * (np.abs(W64) + np.abs(V64) @ (np.abs(V64.T @ W64) + e1)))
    # (4) orthonormal V: what is left of V in the result, over both products
    if n >= m:
        assert np.all(np.abs(V64.T @ Wo.astype(np.float64)) <= (n + m + 2) * U * aG)


# ------------------------------------------------------------------------------------------------------------------ apply_sym_op
def stochastic_graph(n, seed):
    """Row-stochastic P (fp32 values) of a small random graph; one row without neighbours."""
    rng = np.random.RandomState(seed)
    deg = rng.randint(1, 12, n); deg[n // 3] = 0
    rp = np.zeros(n + 1, np.int64); rp[1:] = np.cumsum(deg)
    ci = np.concatenate([rng.choice(n, d, replace=False) for d in deg]).astype(np.int32)
    va = rng.rand(len(ci)) + 0.1
    for i in range(n):
        va[rp[i]:rp[i + 1]] /= max(va[rp[i]:rp[i + 1]].sum(), 1e-300)
    va = va.astype(np.float32)
    A = sp.csr_matrix((va.astype(np.float64), ci.copy(), rp.copy()), shape=(n, n))       # (copies: scipy sorts a row's columns in place; the kernels get them unsorted)
    return dict(n=n, rp=rp, ci=ci, va=va, A=A, absA=abs(A), deg=deg.astype(np.float64))


@pytest.mark.parametrize('addends', ['none', 'W', 'W2', 'W+W2'])
@pytest.mark.parametrize('cols', [1, 17, 48])
@pytest.mark.parametrize('kind', [0, 2])
def test_apply_sym_op(kind, cols, addends):
    n = 203
    g = graph(n) if kind == 0 else stochastic_graph(n, 5)
    rng = np.random.RandomState(cols)
    X, W, W2 = (rng.randn(n, cols).astype(np.float32) for _ in range(3))
    alpha, wa, wb = f32(1.7), f32(-0.8), f32(-1.0)
    if 'W' not in addends.split('+'):
        W = None
    if 'W2' not in addends:
        W2 = None
    if kind == 0 and W is None:
        wa = 1.0                                                                   # (the solvers' own call without addends: wa = 1)
    ldx, ldw, ldw2, ldo = cols + 1, cols + 2, cols + 3, cols + 4
    Out = np.full((n, ldo), SENT, np.float32)
    _hip.check(_hip.lib().gemhip_test_hope_sym_op(n, len(g['ci']), _hip.ptr(g['rp'], C.c_int64), _hip.ptr(g['ci'], C.c_int32), fp(g['va']), kind, alpha,
                                                  fp(padded(X, ldx)), ldx, cols, wa, None if W is None else fp(padded(W, ldw)), ldw, wb,
                                                  None if W2 is None else fp(padded(W2, ldw2)), ldw2, fp(Out), ldo))
    assert_padding(Out, 0, cols)
    if kind == 0:
        ref, bound = spmm_ref(g, alpha, X, wa, W, wb, W2)
    else:
        # Op = N^T N, N = I - P, as two SpMMs:  T = X - P X  (error d1, one SpMM bound)  and  Out = alpha (T - P^T T) + Z,  Z = wa W + wb W2 from a
        # three-flop lincomb (error dz).  The second product's own bound is taken at its actual inputs (|T| + d1, |Z| + dz), and the errors those
        # inputs carry pass through it linearly: |alpha| (I + |P^T|) d1 + dz.
        X64 = X.astype(np.float64); P, aP = g['A'], g['absA']
        degT = np.asarray((P != 0).sum(axis=0)).ravel().astype(np.float64)
        T = X64 - P @ X64
        d1 = (g['deg'][:, None] + 4) * U * (np.abs(X64) + aP @ np.abs(X64))
        Z = (0 if W is None else wa * W.astype(np.float64)) + (0 if W2 is None else wb * W2.astype(np.float64)) + np.zeros_like(X64)
        aZ = (0 if W is None else abs(wa) * np.abs(W).astype(np.float64)) + (0 if W2 is None else abs(wb) * np.abs(W2).astype(np.float64)) + np.zeros_like(X64)
        dz = 3 * U * aZ
        ref = alpha * (T - P.T @ T) + Z
        aT = np.abs(T) + d1
        bound = (degT[:, None] + 4) * U * (abs(alpha) * (aT + aP.T @ aT) + aZ + dz) + abs(alpha) * (d1 + aP.T @ d1) + dz
        dense = np.eye(n) - P.toarray()
        assert np.allclose(ref, alpha * (dense.T @ dense @ X64) + Z, rtol=0, atol=1e-12 * np.abs(ref).max())   # the reference itself: dense (I-P)^T (I-P) X
    err = np.abs(Out[:, :cols] - ref)
    assert np.all(err <= bound), 'error %.3g over the bound' % (err - bound).max()


# ------------------------------------------------------------------------------------------------------------------ lincomb, randn
@pytest.mark.parametrize('n,b', [(1, 1), (7, 3), (1000, 18), (203, 130)])
def test_lincomb(n, b):
    rng = np.random.RandomState(n + b)
    X, Y, Z = (rng.randn(n, b).astype(np.float32) for _ in range(3))
    a, b2, c = f32(0.3), f32(-1.0), f32(2.5)
    ldx, ldy, ldz, ldo = b + 1, b + 2, b + 3, b + 4
    ref = a * X.astype(np.float64) + b2 * Y.astype(np.float64) + c * Z.astype(np.float64)
    bound = 3 * U * (abs(a) * np.abs(X) + abs(b2) * np.abs(Y) + abs(c) * np.abs(Z)).astype(np.float64)        # two products' roundings beyond the fused ones + two sums
    Out = np.full((n, ldo), SENT, np.float32)
    _hip.check(_hip.lib().gemhip_test_hope_lincomb(n, b, a, fp(padded(X, ldx)), ldx, b2, fp(padded(Y, ldy)), ldy, c, fp(padded(Z, ldz)), ldz, 0, fp(Out), ldo))
    assert np.all(np.abs(Out[:, :b] - ref) <= bound)
    assert_padding(Out, 0, b)
    Oi = padded(X, ldo)                                                            # Out IS X (the power iterations' x = z / |z| writes into its own block)
    _hip.check(_hip.lib().gemhip_test_hope_lincomb(n, b, a, None, 0, b2, fp(padded(Y, ldy)), ldy, c, fp(padded(Z, ldz)), ldz, 1, fp(Oi), ldo))
    assert np.array_equal(Oi, Out)


def run_randn(n, b, ld, seed):
    X = np.full((n, ld), SENT, np.float32)
    _hip.check(_hip.lib().gemhip_test_hope_randn(n, b, ld, seed, fp(X)))
    return X


@pytest.mark.parametrize('n,b,ld', [(1, 1, 1), (7, 3, 5), (1000, 18, 20)])
def test_randn(n, b, ld):
    X = run_randn(n, b, ld, 20260923)
    Z = X[:, :b].astype(np.float64)
    assert np.all(np.isfinite(Z)) and np.all(np.abs(Z) < 6.0)                      # every logical element written (the sentinel is far outside)
    assert_padding(X, 0, b)
    assert np.array_equal(run_randn(n, b, ld, 20260923).view(np.uint32), X.view(np.uint32))
    assert not np.array_equal(run_randn(n, b, ld, 20260924)[:, :b], X[:, :b])
    if ld > b:
        assert np.array_equal(run_randn(n, b, b, 20260923), X[:, :b])              # the draws depend on (row, column), not on the leading dimension
    if n * b >= 18000:                                                              # a fixed 4-sigma band for a fixed seed: deterministic
        N = n * b
        assert abs(Z.mean()) <= 4 / np.sqrt(N)
        assert abs(Z.var() - 1) <= 4 * np.sqrt(2.0 / N)
