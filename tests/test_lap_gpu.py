"""Laplacian Eigenmaps on the GPU vs the reference golden (tests/karate_res/LaplacianEigenmaps.txt,
asserted with np.allclose in tests/test_karate.py:47-50,76) and the dense oracle."""
import numpy as np
import pytest

from oracle import hope_oracle
from gem_amd.embedding.lap import LaplacianEigenmaps, symmetric_arrays
from conftest import golden_path

pytestmark = pytest.mark.gpu


def align(X, ref):
    X = X.copy()
    for j in range(X.shape[1]):
        if np.dot(X[:, j], ref[:, j]) < 0:
            X[:, j] *= -1
    return X


def test_karate_matches_reference_golden(karate):
    gold = np.loadtxt(golden_path('ref_karate_LaplacianEigenmaps.txt'))
    m = LaplacianEigenmaps(d=2)
    Y = m.learn_embedding(graph=karate, edge_f=None, is_weighted=True, no_python=True)
    assert Y.shape == (34, 2) and m.get_method_name() == 'lap_eigmap_svd'
    assert np.allclose(align(Y, gold), gold, atol=2e-5)
    n, src, dst, w = symmetric_arrays(karate)
    Xo, wo = hope_oracle.lap_eigmap_dense(n, src, dst, w, 2)
    assert np.allclose(m._eigvals, wo, atol=2e-6) and abs(m._eigvals[0]) < 2e-6
    assert m.get_reconstructed_adj(Y)[3, 5] == pytest.approx(m.get_edge_weight(3, 5))


def test_sbm1024_matches_dense_oracle(sbm1024):
    n, src, dst, w = symmetric_arrays(sbm1024)
    for d in (2, 16):
        m = LaplacianEigenmaps(d=d)
        Y = m.learn_embedding(graph=sbm1024)
        Xo, wo = hope_oracle.lap_eigmap_dense(n, src, dst, w, d)
        assert np.allclose(m._eigvals, wo, atol=5e-6)
        # the two community eigenvectors are separated from the bulk: compare them vector by vector
        Ya = align(Y, Xo)
        assert np.abs(Ya[:, :2] - Xo[:, :2]).max() < 2e-4
        # whole subspace: projector distance
        P = Y @ Y.T; Po = Xo @ Xo.T
        assert np.linalg.norm(P - Po) <= 2e-2 * np.sqrt(d)
    with pytest.raises(ValueError):
        LaplacianEigenmaps(d=2).learn_embedding(graph=None)


def test_lle_karate_and_sbm(karate, sbm1024):
    """LLE (lle.py:23-35): reference golden on karate (the reference only asserts abs(mean diff) < 0.3,
    tests/test_karate.py:52-55,78 -- here it is matched vector by vector), dense oracle on SBM-1024."""
    from gem_amd.embedding.lle import LocallyLinearEmbedding
    gold = np.loadtxt(golden_path('ref_karate_LocallyLinearEmbedding.txt'))
    m = LocallyLinearEmbedding(d=2)
    Y = m.learn_embedding(graph=karate, edge_f=None, is_weighted=True, no_python=True)
    assert abs(np.mean(gold - Y)) < 0.3
    assert np.allclose(align(Y, gold), gold, atol=5e-5)
    n, src, dst, w = symmetric_arrays(sbm1024)
    m = LocallyLinearEmbedding(d=8)
    Y = m.learn_embedding(graph=sbm1024)
    Xo, so = hope_oracle.lle_dense(n, src, dst, w, 8)
    # s = sqrt(c - lambda) in fp32: the trivial s=0 comes out as sqrt(eps*c) ~ 3e-4; the others carry full precision
    assert np.allclose(m._singvals[1:], so[1:], atol=2e-6) and m._singvals[0] < 1e-3, (m._singvals, so)
    Ya = align(Y, Xo)
    assert np.abs(Ya[:, :2] - Xo[:, :2]).max() < 1e-3


def test_eigen_path_agrees_with_block_krylov_and_scipy(monkeypatch):
    """From 16384 nodes up Laplacian Eigenmaps runs HOPE's Chebyshev-filtered eigen-path on D^-1/2 A D^-1/2 (hope_solve.hip sym_filter_svd,
    kind 1).  SBM 20000/200000, d=16: eigenvalues of L_sym against scipy eigsh and against the block-Krylov path, community vectors one by
    one, the subspace by its projector."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as sla
    from gem_amd.graph import sbm_graph
    g = sbm_graph(20000, 200000, 8, seed=21)
    n, src, dst, w = symmetric_arrays(g)
    out = {}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)          # a parity test must not trip the solver's own non-convergence warning
        for sym in ('0', '1'):
            monkeypatch.setenv('GEMHIP_HOPE_SYM', sym)
            # the forced block-Krylov leg (not what runs at this size by default): the 8 eigenvalues at the bottom of this spectrum are clustered within
            # 2e-3 and the fp32 Ritz values stop moving at ~1.5e-6 relative (measured: 1.47e-6 after 30 restarts) -- its tolerance is stated just above
            # that floor instead of the 1e-6 default, with restarts to spare
            m = LaplacianEigenmaps(d=16) if sym == '1' else LaplacianEigenmaps(d=16, tol=2e-6, max_restarts=60)
            Y = m.learn_embedding(graph=g)
            out[sym] = (Y, m._eigvals.copy(), m._stats['solver'])
        monkeypatch.delenv('GEMHIP_HOPE_SYM')
        m = LaplacianEigenmaps(d=16); m.learn_embedding(graph=g)
    assert out['0'][2] == 'block_krylov' and out['1'][2] == 'symmetric_chebyshev_filter' and m._stats['solver'] == 'symmetric_chebyshev_filter'
    A = sp.csr_matrix((np.ones(len(src)) if w is None else w.astype(np.float64), (src, dst)), shape=(n, n))
    deg = np.asarray(A.sum(axis=1)).ravel(); dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1e-300)), 0.0)
    M = sp.diags(dinv) @ A @ sp.diags(dinv)
    ref = 1.0 - np.sort(sla.eigsh(M, k=17, which='LA', tol=1e-10)[0])[::-1]            # eigenvalues of L_sym ascending
    for key in ('0', '1'):          # (the forced block-Krylov leg stops at twice the default tolerance: twice the bar)
        assert np.allclose(out[key][1], ref, atol=2e-5 if key == '0' else 1e-5), (key, np.abs(out[key][1] - ref).max())
    Y0, Y1 = out['0'][0], out['1'][0]
    Ya = align(Y1, Y0)
    assert np.abs(Ya[:, :7] - Y0[:, :7]).max() < 5e-4                                 # the 7 non-trivial community vectors
    assert np.linalg.norm(Y0 @ (Y0.T @ Y1) - Y1) <= 5e-2 * np.sqrt(16)                 # same subspace


def test_lle_eigen_path_at_20k(monkeypatch):
    """From 16384 nodes up LLE runs the Chebyshev-filtered eigen-path on N^T N, N = I - D^-1 A (hope_solve.hip sym_filter_svd kind 2: the
    SMALLEST eigenvalues, two SpMMs per application).  SBM 20000/200000, d=16: every returned pair satisfies ||N v|| = s and
    N^T N v = s^2 v, V is orthonormal, the constant vector comes first (s = 0), the 7 community singular values equal the ones the numpy
    mirror of the solver converged to on the CPU (which agrees with scipy svds(which='SM') at 2000 nodes to 2e-6), and the block-Krylov
    path, where it converges (those 8 values), gives the same numbers."""
    import scipy.sparse as sp
    from gem_amd.embedding.lle import LocallyLinearEmbedding
    from gem_amd.graph import sbm_graph
    g = sbm_graph(20000, 200000, 8, seed=21)
    n, src, dst, w = symmetric_arrays(g)
    out = {}
    for sym in ('0', '1'):
        monkeypatch.setenv('GEMHIP_HOPE_SYM', sym)
        m = LocallyLinearEmbedding(d=16)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)            # the block-Krylov path runs out of restarts here
            Y = m.learn_embedding(graph=g)
        out[sym] = (Y, m._singvals.copy(), m._stats['solver'], dict(m._stats))
    assert out['0'][2] == 'block_krylov' and out['1'][2] == 'symmetric_chebyshev_filter'
    assert out['1'][3]['last_sigma_change'] < 1e-6                                    # converged
    s = out['1'][1]                                                                   # d + 1 values ascending; column 0 is dropped from Y
    mirror = np.array([0.154067107, 0.155979128, 0.165448018, 0.169363148, 0.178480677, 0.183468668, 0.186955405])
    assert s[0] < 2e-3 and np.all(np.diff(s) >= -1e-7)
    assert np.allclose(s[1:8], mirror, atol=2e-5), np.abs(s[1:8] - mirror).max()
    assert np.allclose(out['0'][1][1:8], mirror, atol=2e-4)
    A = sp.csr_matrix((np.ones(len(src)) if w is None else w.astype(np.float64), (src, dst)), shape=(n, n))
    deg = np.asarray(np.abs(A).sum(axis=1)).ravel()
    N = sp.identity(n) - sp.diags(np.where(deg > 0, 1.0 / np.maximum(deg, 1e-300), 0.0)) @ A
    V = out['1'][0]                                                                   # columns 1..d
    NV = N @ V
    assert np.allclose(np.linalg.norm(NV, axis=0), s[1:], atol=2e-5)
    assert np.linalg.norm(N.T @ NV - V * s[1:] ** 2, axis=0).max() < 2e-3
    assert np.abs(V.T @ V - np.eye(16)).max() < 5e-5
    assert np.abs(V.sum(axis=0)).max() / np.sqrt(n) < 5e-3                            # orthogonal to the dropped constant vector
