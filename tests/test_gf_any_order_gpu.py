"""GPU tests of GF on any edge order (gemhip_gf_plan_create_any_order, gf_sweep_units_kernel, GraphFactorization(exact_edge_order=True)):
the unit schedule against the CPU oracle's sequential loop over the SAME order, with test_gf_gpu.py's bound; bit identity against the row
schedule where both exist, of the fused small levels against the level loop, and of two runs; the plugin kwarg."""
import ctypes as C

import numpy as np
import pytest

import oracle
from gem_amd import _hip
from gem_amd.embedding.gf import GraphFactorization
from gem_amd.graph import EdgeListGraph, edge_arrays
from test_gf_any_order import REFUSAL, schedule, shuffled, two_sorted_halves
from test_gf_gpu import assert_close

pytestmark = pytest.mark.gpu


def create(n, src, dst, w, d, flags=0, any_order=True):
    L = _hip.lib(); plan = C.c_void_p()
    src = _hip.as_i32(src); dst = _hip.as_i32(dst); w = _hip.as_f32(w)
    if any_order:
        _hip.check(L.gemhip_gf_plan_create_any_order(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(w, C.c_float), d, flags,
                                                     C.byref(plan)))
    else:
        _hip.check(L.gemhip_gf_plan_create(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(w, C.c_float), d, 0, n, C.byref(plan)))
    return plan


def run(plan, X0, sweeps, eta, regu):
    """Set the table, sweep (in two calls when there is more than one sweep: the current table carries over), fetch."""
    L = _hip.lib()
    X0 = np.ascontiguousarray(X0, dtype=np.float32)
    _hip.check(L.gemhip_gf_plan_set_embedding(plan, _hip.ptr(X0, C.c_float)))
    _hip.check(L.gemhip_gf_plan_sweeps(plan, sweeps - sweeps // 2, eta, regu, None))
    _hip.check(L.gemhip_gf_plan_sweeps(plan, sweeps // 2, eta, regu, None))
    X = np.empty_like(X0)
    _hip.check(L.gemhip_gf_plan_get_embedding(plan, _hip.ptr(X, C.c_float)))
    return X


def info_of(plan):
    info = (C.c_int64 * 8)()
    _hip.check(_hip.lib().gemhip_gf_plan_info(plan, info))
    return list(info)


def train(n, src, dst, w, d, eta, regu, sweeps, X0, flags=0, fused=None):
    plan = create(n, src, dst, w, d, flags)
    try:
        if fused is not None:
            _hip.check(_hip.lib().gemhip_gf_plan_set_fused_levels(plan, fused))
        return run(plan, X0, sweeps, eta, regu), info_of(plan)
    finally:
        _hip.lib().gemhip_gf_plan_destroy(plan)


def assert_unit_plan(info, n, src, dst, d):
    units, levels = schedule(n, src, dst)[3]
    assert info[7] == 1 and info[1] == units and info[2] == levels and info[0] == int((np.asarray(dst) > np.asarray(src)).sum())
    assert info[3] == n and info[4] == d and info[6] == 1


# ---- against the oracle's sequential loop over the same order
def test_the_list_the_row_schedule_refuses():
    n, src, dst = REFUSAL
    X0 = 0.3 * np.random.RandomState(0).randn(n, 8)
    X, info = train(n, src, dst, None, 8, 0.05, 0.01, 25, X0)
    assert_unit_plan(info, n, src, dst, 8)
    assert info[1] == 3 and info[2] == 3
    assert_close(X, oracle.gf_train_f32(n, src, dst, None, 8, 0.05, 0.01, 25, X0))


@pytest.mark.parametrize('d', [2, 7, 128, 130, 512])
def test_karate_shuffled_matches_oracle(karate, d):
    n, src, dst, w = shuffled(*edge_arrays(karate)[:4], seed=1)
    X0 = 0.1 * np.random.RandomState(d).randn(n, d)
    X, info = train(n, src, dst, w, d, 0.05, 0.01, 25, X0)
    assert_unit_plan(info, n, src, dst, d)
    assert info[2] > 1
    assert_close(X, oracle.gf_train_f32(n, src, dst, w, d, 0.05, 0.01, 25, X0))


@pytest.mark.parametrize('sweeps', [1, 2, 3])
def test_sbm1024_shuffled_random_weights_matches_oracle(sbm1024, sweeps):
    """Odd and even sweep counts: the current table is either of the two."""
    n, src, dst, _ = shuffled(*edge_arrays(sbm1024)[:4], seed=2)
    w = (np.random.RandomState(6).rand(len(src)) * 2).astype(np.float32)
    X0 = 0.01 * np.random.RandomState(5).randn(n, 32)
    X, info = train(n, src, dst, w, 32, 0.02, 0.01, sweeps, X0)
    assert_unit_plan(info, n, src, dst, 32)
    assert_close(X, oracle.gf_train_f32(n, src, dst, w, 32, 0.02, 0.01, sweeps, X0))


def hub_graph_with_interleaved_reads():
    """test_gf_gpu.py::test_weighted_shuffled_order_graph's 300-node graph (row 3 has 200 extra edges), with reads of row 3 -- edges (k, 3), k < 3 --
    put INTO row 3's run of edges: after 70 of them, after one more, after 150 and after one more."""
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
    a = int(np.flatnonzero(src == 3)[0])
    assert np.all(src[a:a + 200] == 3)
    for off, k in ((151, 0), (150, 2), (71, 1), (70, 0)):              # back to front: earlier offsets stay valid
        src = np.insert(src, a + off, k); dst = np.insert(dst, a + off, 3)
    w = rng.rand(len(src)).astype(np.float32) * 2
    return n, src.astype(np.int32), dst.astype(np.int32), w, rng


def test_hub_row_read_in_the_middle_of_its_edges():
    n, src, dst, w, rng = hub_graph_with_interleaved_reads()
    unit, level, flags, _ = schedule(n, src, dst)
    sizes = np.bincount(unit[unit >= 0])
    hub_units = np.unique(unit[(src == 3) & (unit >= 0)])
    assert sizes[hub_units].max() > 64 and sizes[hub_units].min() == 1 and len(hub_units) >= 4      # long units, a unit of one edge ...
    assert np.any(flags[(src == 3) & (unit >= 0)] & 2)                                            # ... and units that reload row 3 from the working table
    X0 = 0.1 * rng.randn(n, 16)
    X, info = train(n, src, dst, w, 16, 0.05, 0.02, 10, X0)
    assert_unit_plan(info, n, src, dst, 16)
    assert_close(X, oracle.gf_train_f32(n, src, dst, w, 16, 0.05, 0.02, 10, X0))


# ---- bit identity
@pytest.mark.parametrize('gname,d', [('karate', 7), ('karate', 128), ('sbm1024', 32), ('sbm1024', 256)])
def test_forced_unit_schedule_is_bit_identical_to_the_row_plan(gname, d, request):
    """Where both schedules exist they apply the same gf_apply_edge in the same order per row: karate (a multi-level row plan) and SBM-1024 as
    stored (one level).  Without the force bit the any-order creator returns the row plan itself.  set_rows_per_wave / set_fused_sweeps are
    accepted on a unit plan and change nothing."""
    n, src, dst, w, _ = edge_arrays(request.getfixturevalue(gname))
    X0 = 0.01 * np.random.RandomState(3).randn(n, d)
    L = _hip.lib()
    rows = create(n, src, dst, w, d, any_order=False)
    auto = create(n, src, dst, w, d, flags=0)
    forced = create(n, src, dst, w, d, flags=1)
    try:
        assert info_of(auto) == info_of(rows) and info_of(rows)[7] == 0
        assert_unit_plan(info_of(forced), n, src, dst, d)
        _hip.check(L.gemhip_gf_plan_set_rows_per_wave(forced, 8))
        _hip.check(L.gemhip_gf_plan_set_fused_sweeps(forced, 4, 0))
        want = run(rows, X0, 5, 0.02, 0.01)
        assert np.array_equal(run(auto, X0, 5, 0.02, 0.01), want)
        assert np.array_equal(run(forced, X0, 5, 0.02, 0.01), want)
    finally:
        for p in (rows, auto, forced):
            L.gemhip_gf_plan_destroy(p)


@pytest.mark.parametrize('d', [32, 130])
def test_fused_small_levels_are_bit_identical_to_the_level_loop(sbm1024, d):
    """SBM-1024 as two sorted halves: one big level, then dozens of consecutive levels of a few units, which gemhip_gf_plan_set_fused_levels runs in
    one launch of one workgroup with a barrier between levels.  Rows handed from level to level inside that launch must arrive: same bits as the loop."""
    n, src, dst, w = two_sorted_halves(*edge_arrays(sbm1024)[:4], seed=3)
    unit, level, _, (units, levels) = schedule(n, src, dst)
    fire = np.flatnonzero(unit >= 0)
    per_level = np.bincount(level[fire][np.unique(unit[fire], return_index=True)[1]])           # units of each level
    assert levels > 20 and int((per_level <= 16).sum()) > levels // 2            # the shape the fused launch is for
    X0 = 0.01 * np.random.RandomState(5).randn(n, d)
    out = {k: train(n, src, dst, w, d, 0.02, 0.01, 3, X0, fused=k)[0] for k in (0, 4, 16)}
    assert np.array_equal(out[16], out[0]) and np.array_equal(out[4], out[0])
    assert_close(out[0], oracle.gf_train_f32(n, src, dst, w, d, 0.02, 0.01, 3, X0))
    assert _hip.lib().gemhip_gf_plan_set_fused_levels(None, 0) != 0


def test_two_runs_of_the_same_plan_are_bit_identical(sbm1024):
    n, src, dst, w = shuffled(*edge_arrays(sbm1024)[:4], seed=2)
    X0 = 0.01 * np.random.RandomState(5).randn(n, 128)
    plan = create(n, src, dst, w, 128)
    try:
        a = run(plan, X0, 4, 0.02, 0.01)
        b = run(plan, X0, 4, 0.02, 0.01)
    finally:
        _hip.lib().gemhip_gf_plan_destroy(plan)
    assert np.array_equal(a, b) and not np.array_equal(a, X0.astype(np.float32))


# ---- plugin
def test_plugin_exact_edge_order(sbm1024):
    n, src, dst, _ = shuffled(*edge_arrays(sbm1024)[:4], seed=2)
    w = (np.random.RandomState(6).rand(len(src)) * 2).astype(np.float32)
    g = EdgeListGraph(n, src, dst, w)
    kw = dict(d=32, max_iter=3, eta=0.02, regu=0.01, seed=5, device_init=False)
    m = GraphFactorization(exact_edge_order=True, **kw)
    Y = m.learn_embedding(graph=g, is_weighted=True, no_python=True)
    X0 = (0.01 * np.random.RandomState(5).randn(n, 32)).astype(np.float32)           # the draw of seed=5, device_init=False
    assert Y.dtype == np.float64 and Y.shape == (n, 32)
    assert_close(Y, oracle.gf_train_f32(n, src, dst, w, 32, 0.02, 0.01, 3, X0))
    units, levels = schedule(n, src, dst)[3]
    assert m._stats['schedule'] == 'units' and m._stats['units'] == units and m._stats['levels'] == levels
    # without the kwarg: refused, with the message as before
    with pytest.raises(_hip.GemHipError, match='partly updated'):
        GraphFactorization(**kw).learn_embedding(graph=g, is_weighted=True, no_python=True)
    # a unit schedule is a single-device schedule
    with pytest.raises(ValueError, match='single-device'):
        GraphFactorization(exact_edge_order=True, n_gpus=2, **kw).learn_embedding(graph=g, is_weighted=True, no_python=True)
    # a list the row schedule represents: the row plan, and the table of a run without the kwarg
    a = GraphFactorization(exact_edge_order=True, **kw)
    Ya = a.learn_embedding(graph=sbm1024, is_weighted=True, no_python=True)
    assert a._stats['schedule'] == 'rows' and a._stats['levels'] == 1
    assert np.array_equal(Ya, GraphFactorization(**kw).learn_embedding(graph=sbm1024, is_weighted=True, no_python=True))
