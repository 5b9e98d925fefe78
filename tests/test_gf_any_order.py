"""CPU tests of GF's any-order planner (gemhip_gf_any_order_schedule: host code, no HIP call).

For edge lists the row schedule refuses -- and for some it accepts -- the unit schedule is checked three ways: an independent checker of the
ordering every pair of conflicting edges needs, a numpy fp64 emulation that executes the schedule the way the device does (levels one after
another, the units of a level in any order, two tables) against the sequential loop of gf.py:93-100, bit for bit, and the degenerate case
(edges grouped by source, sources ascending: one level, one unit per firing row)."""
import ctypes as C

import numpy as np
import pytest

from gem_amd import _hip
from gem_amd.graph import EdgeListGraph, edge_arrays, row_schedule_represents


def schedule(n, src, dst):
    """-> unit, level, flags (per edge, -1 = does not fire), (units, levels)"""
    src = _hip.as_i32(src); dst = _hip.as_i32(dst)
    m = len(src)
    unit = np.full(m, -7, np.int32); level = np.full(m, -7, np.int32); flags = np.full(m, -7, np.int32)
    counts = np.zeros(2, np.int64)
    _hip.check(_hip.lib().gemhip_gf_any_order_schedule(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(unit, C.c_int32),
                                                       _hip.ptr(level, C.c_int32), _hip.ptr(flags, C.c_int32), _hip.ptr(counts, C.c_int64)))
    return unit, level, flags, (int(counts[0]), int(counts[1]))


# ---- the lists (shared with tests/test_gf_any_order_gpu.py)
REFUSAL = (4, np.array([1, 0, 1], np.int32), np.array([2, 1, 3], np.int32))          # tests/test_capi.py's refusal list


def shuffled(n, src, dst, w, seed):
    perm = np.random.RandomState(seed).permutation(len(src))
    return n, np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]), (None if w is None else np.ascontiguousarray(w[perm]))


def two_sorted_halves(n, src, dst, w, seed):
    """A random half of the edges in stored order, then the other half in stored order: two sorted files concatenated."""
    pick = np.random.RandomState(seed).rand(len(src)) < 0.5
    perm = np.concatenate([np.flatnonzero(pick), np.flatnonzero(~pick)])
    return n, np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]), (None if w is None else np.ascontiguousarray(w[perm]))


def duplicates_far_apart():
    rng = np.random.RandomState(4)
    src = rng.randint(0, 9, 60).astype(np.int32); dst = rng.randint(0, 9, 60).astype(np.int32)
    src[[0, 59]] = 2; dst[[0, 59]] = 5                      # the same firing edge first and last ...
    src[[7, 41]] = 0; dst[[7, 41]] = 2                      # ... and one that reads the row the other writes, twice
    return 9, src, dst


def self_loops_and_non_firing():
    rng = np.random.RandomState(5)
    src = rng.randint(0, 12, 90).astype(np.int32); dst = rng.randint(0, 12, 90).astype(np.int32)
    src[::9] = dst[::9]                                     # self-loops; about half of the rest has dst < src
    return 12, src, dst


def all_lists(karate, sbm1024):
    kn, ks, kd, _, _ = edge_arrays(karate)
    sn, ss, sd, _, _ = edge_arrays(sbm1024)
    return {
        'refusal': REFUSAL,
        'karate_shuffled': shuffled(kn, ks, kd, None, 1)[:3],
        'sbm1024_shuffled': shuffled(sn, ss, sd, None, 2)[:3],
        'sbm1024_two_halves': two_sorted_halves(sn, ss, sd, None, 3)[:3],
        'duplicates': duplicates_far_apart(),
        'self_loops': self_loops_and_non_firing(),
    }


NAMES = ['refusal', 'karate_shuffled', 'sbm1024_shuffled', 'sbm1024_two_halves', 'duplicates', 'self_loops']


# ---- 1. the ordering every conflicting pair needs
def check_schedule(n, src, dst, unit, level, flags):
    """Two firing edges conflict when they touch a common row and one of them writes it IN THE TABLE THE OTHER USES: X_old is never written during
    a sweep, so a read of X_old conflicts with nothing -- but it is only right while the row has not been written.  Per row, in file order:
    a write comes after every earlier write and after every earlier read of X_new[row] (strictly higher level, or the same unit for two writes);
    a read of X_new[row] comes strictly after every earlier write; a read of X_old[row] has no earlier write; a unit loads its own row from
    X_new exactly when an earlier unit wrote it."""
    fire = dst > src
    assert np.all(unit[~fire] == -1) and np.all(level[~fire] == -1) and np.all(flags[~fire] == -1)
    assert np.all(unit[fire] >= 0) and np.all(level[fire] >= 0) and np.all((flags[fire] & ~3) == 0)
    w_level = np.full(n, -1); w_unit = np.full(n, -1); r_level = np.full(n, -1)     # level of the last write / its unit / highest read of X_new so far
    unit_level = {}; unit_row = {}; unit_own = {}; unit_last = {}
    for e in np.flatnonzero(fire):
        i, j, u, lv = int(src[e]), int(dst[e]), int(unit[e]), int(level[e])
        assert unit_level.setdefault(u, lv) == lv and unit_row.setdefault(u, i) == i                # a unit has one level, one row ...
        assert unit_own.setdefault(u, int(flags[e]) & 2) == int(flags[e]) & 2                       # ... and one source of that row
        if flags[e] & 1:
            assert w_level[j] >= 0 and lv > w_level[j], ('read before the write it must see', e)
            r_level[j] = max(r_level[j], lv)
        else:
            assert w_level[j] < 0, ('X_old read of a row already written', e)
        if u == w_unit[i]:                                         # joins the row's latest unit: nobody may have read the row in between
            assert lv == w_level[i] and unit_last[u] < e and r_level[i] < lv, ('a read of the intermediate row would be skipped', e)
        else:
            assert u not in unit_last, ('a unit is one run of the row\'s edges', e)
            assert lv > w_level[i] and lv > r_level[i], ('write not after an earlier write / read', e)
            assert bool(flags[e] & 2) == (w_level[i] >= 0)
        unit_last[u] = e
        w_level[i] = lv; w_unit[i] = u
    return len(unit_level), (max(unit_level.values()) + 1 if unit_level else 0)


def check_pairs_brute_force(src, dst, unit, level, flags):
    """The same property pair by pair (small lists): e before f in file order, both firing."""
    fire = np.flatnonzero(dst > src)
    for a, e in enumerate(fire):
        for f in fire[a + 1:]:
            ordered = level[e] < level[f] or unit[e] == unit[f]
            if src[e] == src[f]:                                   # both write the row
                assert ordered, (e, f)
            if dst[f] == src[e]:                                   # f reads what e wrote: from X_new, later
                assert flags[f] & 1 and level[e] < level[f], (e, f)
            if dst[e] == src[f] and flags[e] & 1:                  # f overwrites the X_new version e read
                assert level[e] < level[f], (e, f)


@pytest.mark.parametrize('name', NAMES)
def test_conflicting_edges_are_ordered(name, karate, sbm1024):
    n, src, dst = all_lists(karate, sbm1024)[name]
    unit, level, flags, (units, levels) = schedule(n, src, dst)
    assert check_schedule(n, src, dst, unit, level, flags) == (units, levels)
    if len(src) < 200:
        check_pairs_brute_force(src, dst, unit, level, flags)
    if name == 'refusal':
        assert (units, levels) == (3, 3)
        assert unit.tolist() == [0, 1, 2] and level.tolist() == [0, 1, 2] and flags.tolist() == [0, 1, 2]
    assert not row_schedule_represents(src, dst) or name in ('duplicates', 'self_loops')


# ---- 2. executing the schedule == the sequential loop, bit for bit (fp64)
def step(x, xj, w, eta, regu):
    return x - eta * (regu * x - (w - float((x * xj).sum())) * xj)          # gf.py:97-99; d < 8: numpy adds the d products left to right


def sequential(n, src, dst, w, X0, eta, regu, sweeps):
    X = X0.copy()
    for _ in range(sweeps):
        for e in range(len(src)):
            i, j = src[e], dst[e]
            if j > i:
                X[i] = step(X[i].copy(), X[j], w[e], eta, regu)
    return X


def emulate(n, src, dst, w, X0, eta, regu, sweeps, unit, level, flags):
    """What the device does: X_old is read only; level by level, every unit of the level sees the tables as they stood when the level began
    (a snapshot of X_new), the units run in REVERSED order; the tables swap after the sweep."""
    Xold, Xnew = X0.copy(), X0.copy()
    fire = np.flatnonzero(unit >= 0)
    units = {}
    for e in fire:
        units.setdefault(int(unit[e]), []).append(int(e))
    by_level = {}
    for u, es in units.items():
        by_level.setdefault(int(level[es[0]]), []).append(u)
    for _ in range(sweeps):
        for lv in sorted(by_level):
            snap = Xnew.copy()
            for u in reversed(by_level[lv]):
                es = units[u]
                i = src[es[0]]
                x = (snap if flags[es[0]] & 2 else Xold)[i].copy()
                for e in es:
                    x = step(x, (snap if flags[e] & 1 else Xold)[dst[e]], w[e], eta, regu)
                Xnew[i] = x
        Xold, Xnew = Xnew, Xold
    return Xold


@pytest.mark.parametrize('name', NAMES)
def test_schedule_executed_in_fp64_equals_the_sequential_loop(name, karate, sbm1024):
    n, src, dst = all_lists(karate, sbm1024)[name]
    rng = np.random.RandomState(11)
    w = rng.rand(len(src)) * 2
    X0 = 0.3 * rng.randn(n, 4)
    unit, level, flags, _ = schedule(n, src, dst)
    want = sequential(n, src, dst, w, X0, 0.05, 0.02, 3)
    got = emulate(n, src, dst, w, X0, 0.05, 0.02, 3, unit, level, flags)
    assert not np.array_equal(want, X0)
    assert np.array_equal(got, want)


# ---- 3. the degenerate case
def test_grouped_by_ascending_source_is_one_level_and_one_unit_per_row(karate, sbm1024):
    sn, ss, sd, _, _ = edge_arrays(sbm1024)                       # stored: nodes 0..1023, edges by source
    lists = [(sn, ss, sd)]
    for n, src, dst in (all_lists(karate, sbm1024)[k] for k in ('karate_shuffled', 'duplicates', 'self_loops')):
        order = np.argsort(src, kind='stable')
        lists.append((n, src[order], dst[order]))
    for n, src, dst in lists:
        unit, level, flags, (units, levels) = schedule(n, src, dst)
        fire = dst > src
        assert levels == 1 and units == len(np.unique(src[fire]))
        assert np.all(level[fire] == 0) and np.all(flags[fire] == 0)
        assert np.array_equal(np.unique(unit[fire], return_inverse=True)[1], np.unique(src[fire], return_inverse=True)[1])
        assert row_schedule_represents(src, dst)


def test_inspector_validates_and_accepts_null_outputs():
    L = _hip.lib()
    n, src, dst = REFUSAL
    counts = np.zeros(2, np.int64)
    _hip.check(L.gemhip_gf_any_order_schedule(n, 3, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), None, None, None, _hip.ptr(counts, C.c_int64)))
    assert counts.tolist() == [3, 3]
    bad = np.array([0, 9, 1], np.int32)
    assert L.gemhip_gf_any_order_schedule(n, 3, _hip.ptr(src, C.c_int32), _hip.ptr(bad, C.c_int32), None, None, None, None) == _hip.E_INVALID
    assert b'outside' in L.gemhip_last_error()
    e = np.zeros(0, np.int32)
    _hip.check(L.gemhip_gf_any_order_schedule(5, 0, _hip.ptr(e, C.c_int32), _hip.ptr(e, C.c_int32), None, None, None, _hip.ptr(counts, C.c_int64)))
    assert counts.tolist() == [0, 0]


def test_any_order_creator_validates_before_any_device_call():
    L = _hip.lib()
    n, src, dst = REFUSAL
    plan = C.c_void_p()
    for d, flags in ((0, 0), (1026, 0), (513, 0), (8, 2)):
        rc = L.gemhip_gf_plan_create_any_order(n, 3, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), None, d, flags, C.byref(plan))
        assert rc == _hip.E_INVALID and not plan.value
    assert L.gemhip_gf_plan_set_fused_levels(None, 16) == _hip.E_INVALID


def test_exact_edge_order_on_several_gpus_refuses_a_unit_schedule_on_the_host():
    """A unit schedule is a single-device schedule: the plugin says so before any device call (this test runs without a GPU)."""
    from gem_amd.embedding.gf import GraphFactorization
    n, src, dst = REFUSAL
    m = GraphFactorization(d=8, eta=0.05, regu=0.01, max_iter=1, exact_edge_order=True, n_gpus=2, virtual_ranks=True)
    with pytest.raises(ValueError, match='single-device'):
        m.learn_embedding(graph=EdgeListGraph(n, src, dst))
