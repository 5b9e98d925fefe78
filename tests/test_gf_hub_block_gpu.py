"""GPU tests of GF's blocked hub rows (gemhip_gf_plan_set_hub_block: gf_hub_block_kernel applies B edges of a hub row with one Gram matrix on the
fp32 matrix units, B scalar steps and one GEMV), through the C ABI like tests/test_gf_gpu.py.  The mode is not bit-identical to the row kernels; its
bound is theirs: RTOL of max|ref| against the sequential fp32 loop (oracle.gf_train_f32).  The hub threshold is lowered with GEMHIP_GF_HUB_EDGES
(read per plan creation) so that small graphs have hub rows."""
import ctypes as C

import numpy as np
import pytest

import oracle
from gem_amd import _hip
from gem_amd.embedding.gf import GraphFactorization
from gem_amd.graph import edge_arrays, rmat_graph

pytestmark = pytest.mark.gpu

RTOL = 2e-5          # tests/test_gf_gpu.py's


def run(n, src, dst, w, d, eta, regu, sweeps, X0, block=None, unit_plan=False):
    """-> (table after `sweeps` sweeps, B in effect, hub rows, levels).  block: None = leave the plan as created, else gemhip_gf_plan_set_hub_block's
    arguments in turn (an int or a tuple of ints)."""
    L = _hip.lib()
    plan = C.c_void_p()
    edges = (n, len(src), _hip.ptr(_hip.as_i32(src), C.c_int32), _hip.ptr(_hip.as_i32(dst), C.c_int32), _hip.ptr(_hip.as_f32(w), C.c_float), d)
    if unit_plan:
        _hip.check(L.gemhip_gf_plan_create_any_order(*edges, 1, C.byref(plan)))
    else:
        _hip.check(L.gemhip_gf_plan_create(*edges, 0, n, C.byref(plan)))
    try:
        for on in (() if block is None else (block,) if isinstance(block, int) else block):
            _hip.check(L.gemhip_gf_plan_set_hub_block(plan, on))
        b = C.c_int32(-1); hubs = C.c_int64(-1)
        _hip.check(L.gemhip_gf_plan_hub_block(plan, C.byref(b), C.byref(hubs)))
        info = (C.c_int64 * 8)()
        _hip.check(L.gemhip_gf_plan_info(plan, info))
        X = np.ascontiguousarray(X0, dtype=np.float32).copy()
        _hip.check(L.gemhip_gf_plan_set_embedding(plan, _hip.ptr(X, C.c_float)))
        _hip.check(L.gemhip_gf_plan_sweeps(plan, sweeps, eta, regu, None))
        _hip.check(L.gemhip_gf_plan_get_embedding(plan, _hip.ptr(X, C.c_float)))
    finally:
        L.gemhip_gf_plan_destroy(plan)
    return X, b.value, hubs.value, info[2]


def assert_close(X, ref, what=''):
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = float(np.abs(X.astype(np.float64) - ref.astype(np.float64)).max())
    print('%s max|diff| = %.3e of scale %.3e (%.2e relative, bound %.0e)' % (what, err, scale, err / scale, RTOL))
    assert np.isfinite(X).all(), what
    assert err <= RTOL * scale, '%s max|diff|=%.3e vs scale %.3e' % (what, err, scale)


def block_size(d):
    X, b, _, _ = run(2, [0], [1], None, d, 0.1, 0.1, 0, np.zeros((2, d), np.float32), block=1)
    return b


@pytest.fixture(scope='module')
def rmat13():
    n, src, dst, w, _ = edge_arrays(rmat_graph(13, 131072, seed=7))
    assert np.all(np.diff(src) >= 0)                          # ascending sources: a single-level plan
    return n, src, dst, w


@pytest.mark.parametrize('d', [2, 7, 16, 64, 128, 130, 256, 512, 65, 129, 257, 514, 1024])
def test_every_width_matches_the_oracle(d, karate, sbm1024, monkeypatch):
    """Every (floats per lane, chunks) instantiation and both block sizes, on karate (multi-level: hub rows that read X_new) and SBM-1024 with most rows
    hub rows (threshold 3: partial blocks everywhere, rows shorter than one block), at the hyper-parameters of the existing hub-kernel test."""
    monkeypatch.setenv('GEMHIP_GF_HUB_EDGES', '3')
    monkeypatch.delenv('GEMHIP_GF_NO_HUB_KERNEL', raising=False)
    for name, G, sweeps in (('sbm1024', sbm1024, 3), ('karate', karate, 5)):
        n, src, dst, w, _ = edge_arrays(G)
        X0 = (0.01 * np.random.RandomState(3).randn(n, d)).astype(np.float32)
        X, b, hubs, levels = run(n, src, dst, w, d, 0.01, 0.01, sweeps, X0, block=1)
        assert b in (16, 32) and hubs > 0 and (levels > 1) == (name == 'karate')
        assert_close(X, oracle.gf_train_f32(n, src, dst, w, d, 0.01, 0.01, sweeps, X0), '%s d=%d B=%d' % (name, d, b))


@pytest.mark.parametrize('d', [16, 128])
def test_block_boundaries(d, monkeypatch):
    """Rows 0..6 with exactly 1, B-1, B, B+1, 2B, 2B+3 and 5B+1 firing edges (B from the getter): no block, a block short of one edge, exactly one, one
    and an edge, two, two and a partial one, many.  Random weights with zeros and negative ones; row 5 lists one neighbour twice, in two different
    blocks (the planner takes such a list in the default mode too: the default table is compared with the oracle as well).  Threshold 1: every row
    is a hub row."""
    monkeypatch.setenv('GEMHIP_GF_HUB_EDGES', '1')
    monkeypatch.delenv('GEMHIP_GF_NO_HUB_KERNEL', raising=False)
    B = block_size(d)
    counts = [1, B - 1, B, B + 1, 2 * B, 2 * B + 3, 5 * B + 1]
    n = 7 + 5 * B + 40
    rs = np.random.RandomState(d)
    src, dst = [], []
    for i, c in enumerate(counts):
        nb = rs.permutation(np.arange(7, n))[:c]
        if i == 5:
            nb[B + 5] = nb[2]
        src += [i] * c; dst += list(nb)
    src = np.array(src, np.int32); dst = np.array(dst, np.int32)
    w = rs.randn(len(src)).astype(np.float32)
    w[::5] = 0.0
    assert (w < 0).any() and (w == 0).any()
    X0 = (0.1 * rs.randn(n, d)).astype(np.float32)
    ref = oracle.gf_train_f32(n, src, dst, w, d, 0.05, 0.02, 4, X0)
    X, b, hubs, _ = run(n, src, dst, w, d, 0.05, 0.02, 4, X0, block=1)
    assert (b, hubs) == (B, 7)
    assert_close(X, ref, 'boundaries d=%d blocked' % d)
    assert np.array_equal(X[7:], X0[7:])
    assert_close(run(n, src, dst, w, d, 0.05, 0.02, 4, X0)[0], ref, 'boundaries d=%d default' % d)


@pytest.mark.parametrize('regu', [1.0, 0.0])
def test_long_row_has_no_systematic_error(regu):
    """Node 0 with 3000 firing edges at d = 128, eta = 1e-4, X0 = 0.01 randn, 5 sweeps, default threshold.  With regu = 1 the row decays by a = 1 - 1e-4
    per edge: powers of a built by repeated fp32 multiplication by fl32(a) are off by 2e-4 of the row here (numpy fp32 emulation, DESIGN.md
    "GF: blocked hub rows"), ten times the bound; the table of exact powers keeps the kernel inside it."""
    n, m, d = 3100, 3000, 128
    rs = np.random.RandomState(12)
    src = np.zeros(m, np.int32); dst = rs.permutation(np.arange(1, n))[:m].astype(np.int32)
    X0 = (0.01 * rs.randn(n, d)).astype(np.float32)
    X, b, hubs, _ = run(n, src, dst, None, d, 1e-4, regu, 5, X0, block=1)
    assert b > 0 and hubs == 1
    ref = oracle.gf_train_f32(n, src, dst, None, d, 1e-4, regu, 5, X0)
    assert float(np.abs(ref[0] - X0[0]).max()) > 10 * RTOL * float(np.abs(ref).max())    # the row moved by far more than the bound
    print('row 0 on its own scale: %.2e' % (float(np.abs(X[0].astype(np.float64) - ref[0]).max()) / float(np.abs(ref[0]).max())))
    assert_close(X, ref, 'long row regu=%g' % regu)


def test_shuffled_weighted_multi_level_graph(monkeypatch):
    """tests/test_gf_gpu.py::test_weighted_shuffled_order_graph's construction (a hub of 200 edges, shuffled node order, random weights) with threshold 64"""
    monkeypatch.setenv('GEMHIP_GF_HUB_EDGES', '64')
    monkeypatch.delenv('GEMHIP_GF_NO_HUB_KERNEL', raising=False)
    rng = np.random.RandomState(9)
    n = 300
    src = rng.randint(0, n, 4000); dst = rng.randint(0, n, 4000)
    hub = np.full(200, 3); hub_dst = rng.permutation(np.arange(4, n))[:200]
    src = np.concatenate([src, hub]); dst = np.concatenate([dst, hub_dst])
    keep = src != dst
    key = np.unique(src[keep].astype(np.int64) * n + dst[keep])
    src, dst = (key // n).astype(np.int32), (key % n).astype(np.int32)
    order = rng.permutation(n); rank = np.empty(n, int); rank[order] = np.arange(n)
    perm = np.lexsort((rng.rand(len(src)), rank[src]))
    src, dst = src[perm], dst[perm]
    w = rng.rand(len(src)).astype(np.float32) * 2
    X0 = 0.1 * rng.randn(n, 16)
    X, b, hubs, levels = run(n, src, dst, w, 16, 0.05, 0.02, 10, X0, block=1)
    assert b > 0 and hubs >= 1 and levels > 3
    assert_close(X, oracle.gf_train_f32(n, src, dst, w, 16, 0.05, 0.02, 10, X0), 'shuffled weighted')


def test_rmat13_matches_the_oracle(rmat13, monkeypatch):
    monkeypatch.setenv('GEMHIP_GF_HUB_EDGES', '64')
    monkeypatch.delenv('GEMHIP_GF_NO_HUB_KERNEL', raising=False)
    n, src, dst, w = rmat13
    X0 = (0.01 * np.random.RandomState(2).randn(n, 128)).astype(np.float32)
    X, b, hubs, levels = run(n, src, dst, w, 128, 1e-2, 1e-2, 4, X0, block=1)
    assert b > 0 and hubs > 0 and levels == 1
    assert_close(X, oracle.gf_train_f32(n, src, dst, w, 128, 1e-2, 1e-2, 4, X0), 'rmat13 (%d hub rows)' % hubs)


def test_only_hub_rows_change_and_the_switch_is_per_plan(rmat13, monkeypatch):
    """On a single-level plan, after one sweep: every row below the threshold is bit-identical to the default mode's and only hub rows differ; switching
    on and off again gives the default table; two blocked runs agree bit for bit; the producer count does not enter the result; a unit plan accepts
    the setter, reports block 0 and trains as before; 2 is not a value."""
    monkeypatch.setenv('GEMHIP_GF_HUB_EDGES', '64')
    monkeypatch.delenv('GEMHIP_GF_NO_HUB_KERNEL', raising=False)
    monkeypatch.delenv('GEMHIP_GF_HUB_BLOCK', raising=False)
    monkeypatch.delenv('GEMHIP_GF_HUB_PRODUCERS', raising=False)
    n, src, dst, w = rmat13
    d = 128
    X0 = (0.01 * np.random.RandomState(2).randn(n, d)).astype(np.float32)
    args = (n, src, dst, w, d, 1e-2, 1e-2, 1, X0)
    default, b0, hubs, levels = run(*args)
    assert b0 == 0 and levels == 1
    is_hub = np.bincount(src[dst > src], minlength=n) >= 64
    assert hubs == int(is_hub.sum()) > 0
    blocked, b, _, _ = run(*args, block=1)
    assert b == block_size(d) > 0
    assert np.array_equal(blocked[~is_hub], default[~is_hub])
    assert (blocked[is_hub] != default[is_hub]).any()                      # the other association of the same sums shows in the last bits
    assert_close(blocked, default, 'one sweep, blocked against default')
    back, b_back, _, _ = run(*args, block=(1, 0))
    assert b_back == 0 and np.array_equal(back, default)
    assert np.array_equal(run(*args, block=1)[0], blocked)
    for producers in ('3', '7'):
        monkeypatch.setenv('GEMHIP_GF_HUB_PRODUCERS', producers)
        assert np.array_equal(run(*args, block=1)[0], blocked), producers
    monkeypatch.delenv('GEMHIP_GF_HUB_PRODUCERS')
    monkeypatch.setenv('GEMHIP_GF_HUB_BLOCK', '1')                         # the initial value of a plan comes from the environment
    from_env, b_env, _, _ = run(*args)
    assert b_env == b and np.array_equal(from_env, blocked)
    monkeypatch.delenv('GEMHIP_GF_HUB_BLOCK')
    units, bu0, _, _ = run(*args, unit_plan=True)
    units_on, bu, _, _ = run(*args, block=1, unit_plan=True)
    assert (bu0, bu) == (0, 0) and np.array_equal(units_on, units) and np.array_equal(units, default)
    L = _hip.lib()
    plan = C.c_void_p()
    e = np.array([0], np.int32); f = np.array([1], np.int32)
    _hip.check(L.gemhip_gf_plan_create(2, 1, _hip.ptr(e, C.c_int32), _hip.ptr(f, C.c_int32), None, 8, 0, 2, C.byref(plan)))
    try:
        assert L.gemhip_gf_plan_set_hub_block(plan, 2) == _hip.E_INVALID
        assert L.gemhip_gf_plan_set_hub_block(plan, -1) == _hip.E_INVALID
    finally:
        L.gemhip_gf_plan_destroy(plan)


def test_plugin_kwarg(rmat13, monkeypatch):
    monkeypatch.setenv('GEMHIP_GF_HUB_EDGES', '64')
    monkeypatch.delenv('GEMHIP_GF_NO_HUB_KERNEL', raising=False)
    from gem_amd.graph import EdgeListGraph
    n, src, dst, w = rmat13
    m = GraphFactorization(d=32, max_iter=4, eta=1e-2, regu=1e-2, hub_block=True, seed=1, device_init=False)
    Y = m.learn_embedding(graph=EdgeListGraph(n, src, dst, None), is_weighted=True, no_python=True)
    assert m._stats['hub_block'] == block_size(32) > 0 and m._stats['hub_rows'] > 0
    X0 = (0.01 * np.random.RandomState(1).randn(n, 32)).astype(np.float32)
    assert Y.dtype == np.float64 and Y.shape == (n, 32)
    assert_close(Y, oracle.gf_train_f32(n, src, dst, w, 32, 1e-2, 1e-2, 4, X0), 'plugin')
