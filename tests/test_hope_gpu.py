"""GPU parity tests for HOPE: device block-Krylov SVD of the implicit Katz operator vs the reference's
golden vector, vs vectors produced by running hope.py, vs the CPU oracle; properties at BASELINE
configs[2] (SBM 100k/1M, d=128)."""
import json

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import hope_oracle
from gem_amd.embedding.hope import HOPE
from gem_amd.evaluation import reconstruction as gr
from gem_amd.graph import edge_arrays, sbm_graph
from conftest import golden_path

pytestmark = pytest.mark.gpu


def katz_apply(A, beta, X, terms=60):
    """S X in fp64 by the Neumann series (CPU check of residuals)."""
    W = beta * (A @ X)
    Z = W.copy()
    for _ in range(terms):
        Z = W + beta * (A @ Z)
    return Z


def test_karate_matches_reference_golden(karate):
    """tests/karate_res/HOPE.txt is the one tight numeric pin of the reference (np.allclose,
    tests/test_karate.py:42-45,76).  fp32 device arithmetic: atol 2e-5 on entries of size ~0.1-0.4."""
    gold = np.loadtxt(golden_path('ref_karate_HOPE.txt'))
    m = HOPE(d=4, beta=0.01)
    Y = m.learn_embedding(graph=karate, edge_f=None, is_weighted=True, no_python=True)
    assert Y.shape == (34, 4) and Y.dtype == np.float64 and m.get_embedding() is Y
    assert np.allclose(np.abs(Y), np.abs(gold), atol=2e-5, rtol=1e-4)
    assert np.allclose(hope_oracle.align_signs(Y, gold, 4), gold, atol=2e-5, rtol=1e-4)
    assert np.all(np.diff(m._sigma) >= 0)                                    # svds order: ascending (hope.py:33)
    # get_edge_weight(i, j) = X[i,:k] . X[j,k:] ~ S_ij (hope.py:43-44)
    n, src, dst, w, order = edge_arrays(karate)
    _, s = hope_oracle.hope_dense(hope_oracle.adjacency(n, src, dst, w, order), 0.01, 4)
    assert np.allclose(m._sigma, s, rtol=2e-5)


@pytest.mark.parametrize('d', [32, 8, 128])
def test_sbm1024_matches_reference_run(sbm1024, d):
    n, src, dst, w, _ = edge_arrays(sbm1024)
    sv = np.load(golden_path('hope_sbm1024_sigma.npy'))
    m = HOPE(d=d, beta=0.01)
    Y = m.learn_embedding(graph=sbm1024, is_weighted=True, no_python=True)
    k = d // 2
    assert np.allclose(m._sigma[::-1], sv[:k], rtol=3e-5), np.abs(m._sigma[::-1] / sv[:k] - 1).max()
    A = hope_oracle.adjacency(n, src, dst, w)
    Xo, so = hope_oracle.hope_dense(A, 0.01, d)
    # the rank-k reconstruction U S V^T is what the embedding encodes: compare it entrywise with the oracle's
    R = Y[:, :k] @ Y[:, k:].T; Ro = Xo[:, :k] @ Xo[:, k:].T
    assert np.linalg.norm(R - Ro) <= 2e-3 * np.linalg.norm(Ro)
    if d == 32:
        gold = np.load(golden_path('hope_sbm1024_d32.npz'))['X']           # produced by running hope.py itself
        Ya = hope_oracle.align_signs(Y, gold, d)
        # per-vector agreement where the spectrum separates them: the 3 community directions
        for j in (k - 1, k - 2, k - 3):
            for half in (0, k):
                c = np.dot(Ya[:, half + j], gold[:, half + j]) / (np.linalg.norm(Ya[:, half + j]) * np.linalg.norm(gold[:, half + j]))
                assert c > 1 - 1e-5
        ref = json.load(open(golden_path('map_ref.json')))['sbm1024_hope_d32']
        MAP = gr.evaluateStaticGraphReconstruction(sbm1024, m, Y, None)[0]
        assert abs(MAP - ref) <= 0.01 * ref, (MAP, ref)


def test_weighted_directed_graph_vs_operator_oracle():
    rng = np.random.RandomState(3)
    n = 3000
    src = rng.randint(0, n, 30000); dst = rng.randint(0, n, 30000)
    keep = src != dst
    key = np.unique(src[keep].astype(np.int64) * n + dst[keep])
    src, dst = (key // n).astype(np.int32), (key % n).astype(np.int32)
    w = (rng.rand(len(src)) + 0.5).astype(np.float32)
    from gem_amd.graph import EdgeListGraph
    g = EdgeListGraph(n, src, dst, w)
    m = HOPE(d=16, beta=0.02)
    Y = m.learn_embedding(graph=g, is_weighted=True)
    A = hope_oracle.adjacency(n, src, dst, w)
    Xo, so = hope_oracle.hope_operator(A, 0.02, 16)
    assert np.allclose(m._sigma, so, rtol=5e-5)
    R = Y[:, :8] @ Y[:, 8:].T; Ro = Xo[:, :8] @ Xo[:, 8:].T
    assert np.linalg.norm(R - Ro) <= 5e-3 * np.linalg.norm(Ro)


def test_error_conventions(karate):
    with pytest.raises(ValueError):
        HOPE(d=4, beta=0.01).learn_embedding(graph=None)
    from gem_amd import _hip
    with pytest.raises(_hip.GemHipError, match='does not converge'):
        HOPE(d=4, beta=0.5).learn_embedding(graph=karate)                    # beta * sigma_max(A) > 1


def test_baseline_config_properties():
    """BASELINE configs[2]: SBM 100k nodes / 1M edges, HOPE d=128 (k=64), beta=0.01."""
    g = sbm_graph(100000, 1000000, 32, seed=20260925)
    n, src, dst, w, _ = edge_arrays(g)
    m = HOPE(d=128, beta=0.01)
    Y = m.learn_embedding(graph=g, is_weighted=True)
    k = 64
    s = m._sigma
    assert Y.shape == (n, 128) and np.isfinite(Y).all() and np.all(np.diff(s) >= 0) and s[0] > 0
    U = Y[:, :k] / np.sqrt(s); V = Y[:, k:] / np.sqrt(s)
    assert np.abs(U.T @ U - np.eye(k)).max() < 5e-5 and np.abs(V.T @ V - np.eye(k)).max() < 5e-5
    A = sp.csr_matrix((np.ones(len(src)), (src, dst)), shape=(n, n))
    # singular-triplet residuals  ||S v - s u|| / s  and  ||S^T u - s v|| / s  for the separated (community) triplets
    idx = [k - 1, k - 2, k - 16, k - 32]
    SV = katz_apply(A, 0.01, V[:, idx]); STU = katz_apply(A.T.tocsr(), 0.01, U[:, idx])
    for c, j in enumerate(idx):
        assert np.linalg.norm(SV[:, c] - s[j] * U[:, j]) <= 2e-3 * s[j]
        assert np.linalg.norm(STU[:, c] - s[j] * V[:, j]) <= 2e-3 * s[j]
    # Ritz values are Rayleigh quotients: u^T S v = s for EVERY returned pair, converged or not
    SVall = katz_apply(A, 0.01, V)
    assert np.allclose(np.einsum('ij,ij->j', U, SVall), s, rtol=2e-4)
    # 32 planted communities -> 32 singular values above the bulk edge
    assert s[k - 32] > 1.15 * s[k - 33]


def test_all_64_singular_values_at_baseline_config_vs_arpack():
    """BASELINE configs[2] (SBM 100k/1M, d=128, beta=0.01): hope.py:33 would return svds(S, k=64).  The CPU answer -- ARPACK on the
    implicit Katz-series operator, tol 1e-9, 76 s (scripts/make_golden_hope_sigma.py; the dense S needs 80 GB) -- is committed as
    tests/golden/hope_sigma_sbm100k.json; every one of the 64 singular values of the HIP solve agrees to 1e-4 relative."""
    ref = json.load(open(golden_path('hope_sigma_sbm100k.json')))
    pr = ref['params']
    g = sbm_graph(pr['n'], pr['edges'], pr['blocks'], pr['seed'])
    m = HOPE(d=pr['d'], beta=pr['beta'])
    m.learn_embedding(graph=g, is_weighted=True, no_python=True)
    s_ref = np.asarray(ref['sigma_ascending'])
    rel = np.abs(np.asarray(m._sigma) / s_ref - 1.0)
    assert rel.max() <= 1e-4, (rel.max(), int(rel.argmax()))


def test_all_64_singular_values_of_the_directed_graph_vs_arpack():
    """The general case of hope.py:28-36 (no symmetry): the same SBM 100k/1M with every undirected edge kept in one random direction
    (gem_amd.graph.orient_randomly, seed 1; bench.py's `hope_sbm100k_directed` workload).  ARPACK svds on the implicit Katz operator,
    tol 1e-9 (scripts/make_golden_hope_sigma.py --directed) vs the HIP block-Krylov solve: all 64 singular values to 1e-4 relative, and
    the solver reports the general path."""
    from gem_amd.graph import orient_randomly
    ref = json.load(open(golden_path('hope_sigma_sbm100k_directed.json')))
    pr = ref['params']
    g = orient_randomly(sbm_graph(pr['n'], pr['edges'], pr['blocks'], pr['seed']), pr['orient_seed'])
    m = HOPE(d=pr['d'], beta=pr['beta'])
    m.learn_embedding(graph=g, is_weighted=True, no_python=True)
    assert m._stats['solver'] == 'block_krylov'
    s_ref = np.asarray(ref['sigma_ascending'])
    rel = np.abs(np.asarray(m._sigma) / s_ref - 1.0)
    assert rel.max() <= 1e-4, (rel.max(), int(rel.argmax()))


def test_symmetric_eigen_path_agrees_with_the_block_krylov_path(monkeypatch):
    """Undirected graphs take the Chebyshev-filtered eigen-path on A (hope_solve.hip sym_filter_svd; automatic from 16384 nodes, forced here
    at 8192): same singular values and the same rank-k reconstruction U S V^T as the general block-Krylov solver on S^T S, which the
    other tests pin against the reference's runs; a directed graph never takes it."""
    g = sbm_graph(8192, 81920, 8, seed=11)
    out = {}
    for sym in ('0', '1'):
        monkeypatch.setenv('GEMHIP_HOPE_SYM', sym)
        m = HOPE(d=32, beta=0.01)
        Y = m.learn_embedding(graph=g, is_weighted=True, no_python=True)
        out[sym] = (Y, m._sigma.copy(), m._stats['solver'])
    assert out['0'][2] == 'block_krylov' and out['1'][2] == 'symmetric_chebyshev_filter'
    assert np.allclose(out['0'][1], out['1'][1], rtol=5e-5), np.abs(out['0'][1] / out['1'][1] - 1).max()
    k = 16
    R0 = out['0'][0][:, :k] @ out['0'][0][:, k:].T; R1 = out['1'][0][:, :k] @ out['1'][0][:, k:].T
    assert np.linalg.norm(R0 - R1) <= 5e-3 * np.linalg.norm(R0)
    # the 8 community triplets are separated: vectors agree one by one (signs are fixed by the same convention on both paths)
    for j in range(k - 1, k - 9, -1):
        for half in (0, k):
            a, b = out['0'][0][:, half + j], out['1'][0][:, half + j]
            assert np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)) > 1 - 1e-4
    # directed graph: the general solver, whatever the switch says
    n, src, dst, w, _ = edge_arrays(g)
    from gem_amd.graph import EdgeListGraph
    keep = src < dst
    gd = EdgeListGraph(n, src[keep], dst[keep], None)
    m = HOPE(d=8, beta=0.01)
    m.learn_embedding(graph=gd, is_weighted=True, no_python=True)
    assert m._stats['solver'] == 'block_krylov'


def test_eigen_path_unfused_rayleigh_ritz_agrees_with_the_fused_one(monkeypatch):
    """GEMHIP_HOPE_SYM_FUSED_RR=0 keeps the two-pass CholeskyQR, the plain Rayleigh-Ritz step and the three-GEMM residuals of the eigen-path
    (the A/B branch of sym_filter_svd, which no other test reaches): same singular values and community vectors as the fused default, at the
    bars test_symmetric_eigen_path_agrees_with_the_block_krylov_path sets between solver paths."""
    g = sbm_graph(2048, 20480, 8, seed=11)
    k = 16
    monkeypatch.setenv('GEMHIP_HOPE_SYM', '1')
    out = {}
    for fused in (None, '0'):
        if fused is None:
            monkeypatch.delenv('GEMHIP_HOPE_SYM_FUSED_RR', raising=False)
        else:
            monkeypatch.setenv('GEMHIP_HOPE_SYM_FUSED_RR', fused)
        m = HOPE(d=2 * k, beta=0.01)
        Y = m.learn_embedding(graph=g, is_weighted=True, no_python=True)
        assert m._stats['solver'] == 'symmetric_chebyshev_filter'
        out[fused] = (Y, m._sigma.copy())
    assert np.allclose(out[None][1], out['0'][1], rtol=5e-5), np.abs(out[None][1] / out['0'][1] - 1).max()
    for j in range(k - 1, k - 9, -1):                      # the 8 separated community triplets, vector by vector
        for half in (0, k):
            a, b = out[None][0][:, half + j], out['0'][0][:, half + j]
            assert np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)) > 1 - 1e-4


def test_symmetric_eigen_path_two_sided_spectrum(monkeypatch):
    """A weighted bipartite graph has the spectrum +-lambda: the k largest |f(lambda)| mix both ends (f(x) = beta x / (1 - beta x) favours
    the positive one), and a negative eigenvalue gives u = -v.  Eigen-path (forced) against the block-Krylov path."""
    from gem_amd.graph import EdgeListGraph
    n = 8192
    rs = np.random.RandomState(5)
    a = rs.randint(0, n // 2, 60000); b = rs.randint(n // 2, n, 60000)
    key = np.unique(a.astype(np.int64) * n + b); a = (key // n).astype(np.int32); b = (key % n).astype(np.int32)
    w = (rs.rand(len(a)) + 0.5).astype(np.float32)
    g = EdgeListGraph(n, np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w]))
    out = {}
    for sym in ('0', '1'):
        monkeypatch.setenv('GEMHIP_HOPE_SYM', sym)
        m = HOPE(d=32, beta=0.01)
        Y = m.learn_embedding(graph=g, is_weighted=True, no_python=True)
        out[sym] = (Y, m._sigma.copy(), m._stats['solver'])
    assert out['1'][2] == 'symmetric_chebyshev_filter' and out['0'][2] == 'block_krylov'
    assert np.allclose(out['0'][1], out['1'][1], rtol=5e-5), np.abs(out['0'][1] / out['1'][1] - 1).max()
    k = 16
    Y = out['1'][0]
    s = out['1'][1]
    # sigma_3 .. sigma_16 sit in the bulk edge (relative gaps ~1e-3): the individual vectors there are not determined to better than
    # residual / gap, so the two solvers are compared on the separated pairs, and every returned triplet is checked on its own:
    # ||S v - sigma u|| and ||S^T u - sigma v|| small, u^T S v = sigma, U and V orthonormal
    for j in (k - 1, k - 2):
        for half in (0, k):
            a0, a1 = out['0'][0][:, half + j], Y[:, half + j]
            assert np.dot(a0, a1) / (np.linalg.norm(a0) * np.linalg.norm(a1)) > 1 - 1e-5
    A = sp.csr_matrix((g.w.astype(np.float64), (g.src, g.dst)), shape=(n, n))
    U = Y[:, :k] / np.sqrt(s); V = Y[:, k:] / np.sqrt(s)
    SV = katz_apply(A, 0.01, V); STU = katz_apply(A.T.tocsr(), 0.01, U)
    assert np.linalg.norm(SV - U * s, axis=0).max() <= 1e-2 * s[0] and np.linalg.norm(STU - V * s, axis=0).max() <= 1e-2 * s[0]
    assert np.allclose(np.einsum('ij,ij->j', U, SV), s, rtol=2e-4)
    assert np.abs(U.T @ U - np.eye(k)).max() < 5e-5 and np.abs(V.T @ V - np.eye(k)).max() < 5e-5
    # Perron pair (largest sigma): u = v;  its mirror -lambda_max (second largest sigma): u = -v
    assert np.allclose(Y[:, k - 1], Y[:, 2 * k - 1], atol=1e-6) and np.allclose(Y[:, k - 2], -Y[:, 2 * k - 2], atol=1e-6)
    lam = s / (0.01 * (1 + s))                                   # f^-1 on the positive side
    assert abs(s[k - 2] - 0.01 * lam[k - 1] / (1 + 0.01 * lam[k - 1])) <= 1e-5 * s[k - 2]   # |f(-lambda_max)|


@pytest.mark.parametrize('sym', ['0', '1'])
def test_device_output_solve_equals_the_host_output_solve(sbm1024, sym, monkeypatch):
    """gemhip_hope_plan_solve_device leaves U sqrt(S) / V sqrt(S) in HBM (what bench.py times: outputs resident); it is the same solve as
    gemhip_hope_plan_solve (hope.py:33-36 semantics, numpy out) -- both solvers (block Krylov, eigen-path), bit for bit -- and it refuses host
    pointers instead of writing through them."""
    import ctypes as C
    from gem_amd import _hip
    from gem_amd.graph import to_csr
    monkeypatch.setenv('GEMHIP_HOPE_SYM', sym)
    L = _hip.lib()
    n, src, dst, w, _ = edge_arrays(sbm1024)
    row_ptr, col, _ = to_csr(n, src, dst, None)
    k = 8
    plan = C.c_void_p()
    _hip.check(L.gemhip_hope_plan_create(n, len(col), _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), None, 0.01, C.byref(plan)))
    U = np.empty((n, k), np.float32); V = np.empty_like(U); s1 = np.empty(k, np.float32); s2 = np.empty(k, np.float32)
    _hip.check(L.gemhip_hope_plan_solve(plan, k, 16, 3, 20, 1e-5, 7, _hip.ptr(U, C.c_float), _hip.ptr(V, C.c_float), _hip.ptr(s1, C.c_float), None))
    dU, dV = C.c_void_p(), C.c_void_p()
    _hip.check(L.gemhip_malloc(C.byref(dU), U.nbytes)); _hip.check(L.gemhip_malloc(C.byref(dV), V.nbytes))
    _hip.check(L.gemhip_hope_plan_solve_device(plan, k, 16, 3, 20, 1e-5, 7, dU, dV, _hip.ptr(s2, C.c_float), None))
    U2 = np.empty_like(U); V2 = np.empty_like(V)
    _hip.check(L.gemhip_memcpy_d2h(U2.ctypes.data_as(C.c_void_p), dU, U.nbytes)); _hip.check(L.gemhip_memcpy_d2h(V2.ctypes.data_as(C.c_void_p), dV, V.nbytes))
    assert np.array_equal(U, U2) and np.array_equal(V, V2) and np.array_equal(s1, s2)
    assert L.gemhip_hope_plan_solve_device(plan, k, 16, 3, 20, 1e-5, 7, U.ctypes.data_as(C.c_void_p), dV, _hip.ptr(s2, C.c_float), None) != 0
    _hip.check(L.gemhip_free(dU)); _hip.check(L.gemhip_free(dV))
    _hip.check(L.gemhip_hope_plan_destroy(plan))
