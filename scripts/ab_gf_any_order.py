"""GF on edge orders the row schedule refuses: microseconds per sweep of the unit schedule (gemhip_gf_plan_create_any_order) with the fused small levels
(gemhip_gf_plan_set_fused_levels) off and on, next to the same edges regrouped by source (regroup_edges=True: the row schedule, another visiting order)
-- the cost of exactness.  d=128; SBM-1024 as two sorted halves (the fixture's shape of interleaving), SBM 10k/100k (BASELINE configs[1]) as two sorted
halves and shuffled.  The settings alternate inside every repetition; min / median / max over the repetitions give the run-to-run spread.
    python scripts/ab_gf_any_order.py [out.json]"""
import ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from gem_amd import _hip
from gem_amd.graph import sbm_graph, edge_arrays, group_edges_by_source

D, SWEEPS, REPS, MAX_UNITS = 128, int(os.environ.get('SWEEPS', 300)), int(os.environ.get('REPS', 7)), 16
L = _hip.lib()


def halves(src, dst, seed):
    pick = np.random.RandomState(seed).rand(len(src)) < 0.5
    perm = np.concatenate([np.flatnonzero(pick), np.flatnonzero(~pick)])
    return np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm])


def shuffle(src, dst, seed):
    perm = np.random.RandomState(seed).permutation(len(src))
    return np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm])


def launches(per_level, max_units):
    """(levels with more than max_units units) + (runs of consecutive smaller levels)"""
    small = per_level <= max_units if max_units > 0 else np.zeros(len(per_level), bool)
    runs = int(small[0]) + int(np.sum(small[1:] & ~small[:-1])) if len(small) else 0
    return int((~small).sum()) + runs


def timed(plan):
    _hip.check(L.gemhip_synchronize(None))
    t0 = time.perf_counter()
    _hip.check(L.gemhip_gf_plan_sweeps(plan, SWEEPS, 1e-4, 1.0, None))
    _hip.check(L.gemhip_synchronize(None))
    return (time.perf_counter() - t0) / SWEEPS * 1e6


def table(plan, n):
    X = np.empty((n, D), np.float32)
    _hip.check(L.gemhip_gf_plan_get_embedding(plan, _hip.ptr(X, C.c_float)))
    return X


def measure(name, n, src, dst):
    m = len(src)
    unit = np.empty(m, np.int32); level = np.empty(m, np.int32); counts = np.zeros(2, np.int64)
    _hip.check(L.gemhip_gf_any_order_schedule(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(unit, C.c_int32), _hip.ptr(level, C.c_int32),
                                              None, _hip.ptr(counts, C.c_int64)))
    fire = np.flatnonzero(unit >= 0)
    per_level = np.bincount(level[fire][np.unique(unit[fire], return_index=True)[1]])
    X0 = (0.01 * np.random.RandomState(1).randn(n, D)).astype(np.float32)
    units = C.c_void_p(); rows = C.c_void_p()
    _hip.check(L.gemhip_gf_plan_create_any_order(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), None, D, 0, C.byref(units)))
    gs, gd, _ = group_edges_by_source(src, dst)
    gs = np.ascontiguousarray(gs, np.int32); gd = np.ascontiguousarray(gd, np.int32)
    _hip.check(L.gemhip_gf_plan_create(n, m, _hip.ptr(gs, C.c_int32), _hip.ptr(gd, C.c_int32), None, D, 0, n, C.byref(rows)))
    info = (C.c_int64 * 8)(); _hip.check(L.gemhip_gf_plan_info(units, info))
    rinfo = (C.c_int64 * 8)(); _hip.check(L.gemhip_gf_plan_info(rows, rinfo))
    assert info[7] == 1 and info[1] == counts[0] and info[2] == counts[1]
    # same bits with the fused levels on and off
    tabs = []
    for k in (0, MAX_UNITS):
        _hip.check(L.gemhip_gf_plan_set_fused_levels(units, k))
        _hip.check(L.gemhip_gf_plan_set_embedding(units, _hip.ptr(X0, C.c_float)))
        _hip.check(L.gemhip_gf_plan_sweeps(units, 50, 1e-4, 1.0, None))              # (also the warm-up)
        tabs.append(table(units, n))
    _hip.check(L.gemhip_gf_plan_set_embedding(rows, _hip.ptr(X0, C.c_float)))
    _hip.check(L.gemhip_gf_plan_sweeps(rows, 50, 1e-4, 1.0, None))
    us = {'level_loop': [], 'fused_levels': [], 'regrouped_rows': []}
    for _ in range(REPS):
        _hip.check(L.gemhip_gf_plan_set_fused_levels(units, 0)); us['level_loop'].append(timed(units))
        _hip.check(L.gemhip_gf_plan_set_fused_levels(units, MAX_UNITS)); us['fused_levels'].append(timed(units))
        us['regrouped_rows'].append(timed(rows))
    L.gemhip_gf_plan_destroy(units); L.gemhip_gf_plan_destroy(rows)
    stat = lambda v: dict(min=round(min(v), 2), median=round(float(np.median(v)), 2), max=round(max(v), 2))
    return dict(list=name, n=n, edges=m, firing_edges=int(info[0]), d=D, units=int(counts[0]), levels=int(counts[1]),
                levels_of_at_most_16_units=int((per_level <= MAX_UNITS).sum()), longest_unit_edges=int(np.bincount(unit[fire]).max()),
                launches_per_sweep=dict(level_loop=launches(per_level, 0), fused_levels=launches(per_level, MAX_UNITS), regrouped_rows=int(rinfo[2])),
                us_per_sweep={k: stat(v) for k, v in us.items()}, fused_bit_identical_to_level_loop=bool(np.array_equal(tabs[0], tabs[1])),
                sweeps_per_timing=SWEEPS, repetitions=REPS)


if __name__ == '__main__':
    _hip.require_device()
    out = []
    e = np.load(os.path.join(ROOT, 'tests', 'golden', 'sbm1024_edges.npy'))
    s1, d1 = np.ascontiguousarray(e[:, 0], np.int32), np.ascontiguousarray(e[:, 1], np.int32)
    n2, s2, d2, _, _ = edge_arrays(sbm_graph(10000, 100000, 10, seed=20260924))
    for name, n, (src, dst) in (('sbm1024_two_sorted_halves', 1024, halves(s1, d1, 3)), ('sbm10k_100k_two_sorted_halves', n2, halves(s2, d2, 3)),
                                ('sbm10k_100k_shuffled', n2, shuffle(s2, d2, 2))):
        r = measure(name, n, src, dst)
        print(json.dumps(r), flush=True)
        out.append(r)
    if len(sys.argv) > 1:
        json.dump(dict(what='GF unit schedule, us per sweep (host clock around SWEEPS sweeps and a device synchronise), MI355X', results=out),
                  open(sys.argv[1], 'w'), indent=1)
