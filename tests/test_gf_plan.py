"""CPU tests of GF's host planning (gem_amd/csrc/gf_plan.hip) as plain C++ behind scripts/asan/gf_plan_driver.cpp: no HIP, no library, no device.

The driver's digests -- acceptance rule, row plan and unit plans (fused_levels 0 / 1 / 16) of edge lists it generates from seeds -- equal
tests/golden/gf_plan_digest.txt, recorded from the planner as it moved out of gf.hip (CHANGELOG.md); and the row plans it writes for lists given
here equal what numpy derives from the reference's visiting order (gf.py:93-100: the edges in file order, a source's row trained when first met)."""
import os
import subprocess

import numpy as np
import pytest

from gem_amd import build
from gem_amd.graph import edge_arrays, row_schedule_represents

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    exe = str(tmp_path_factory.mktemp('gf_plan') / 'gf_plan_driver')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(ROOT, 'gem_amd', 'csrc', 'gf_plan.hip'),
                           os.path.join(ROOT, 'scripts', 'asan', 'gf_plan_driver.cpp'), '-o', exe])
    return exe


def test_driver_reproduces_the_recorded_digests(driver):
    run = subprocess.run([driver, 'digest'], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert run.stdout == open(os.path.join(ROOT, 'tests', 'golden', 'gf_plan_digest.txt'), 'rb').read()


def driver_rows(driver, tmp_path, n, src, dst, w, row_begin, row_end, hub_edges):
    with open(tmp_path / 'in', 'wb') as f:
        np.array([n, len(src), row_begin, row_end, hub_edges, w is not None], np.int64).tofile(f)
        np.ascontiguousarray(src, np.int32).tofile(f); np.ascontiguousarray(dst, np.int32).tofile(f)
        if w is not None:
            np.ascontiguousarray(w, np.float32).tofile(f)
    subprocess.check_call([driver, 'rows', str(tmp_path / 'in'), str(tmp_path / 'out')])
    with open(tmp_path / 'out', 'rb') as f:
        kind, edge, first, last = (int(v) for v in np.fromfile(f, np.int64, 4))
        if kind:
            return dict(kind=kind, edge=edge, first=first, last=last)
        nrows, nupd, nlevels = (int(v) for v in np.fromfile(f, np.int64, 3))
        out = dict(kind=0, rows=np.fromfile(f, np.int32, nrows), ptr=np.fromfile(f, np.int64, nrows + 1), col=np.fromfile(f, np.uint32, nupd),
                   w=np.fromfile(f, np.float32, nupd), level_off=np.fromfile(f, np.int64, nlevels + 1), level_hubs=np.fromfile(f, np.int64, nlevels),
                   level_maxlen=np.fromfile(f, np.int64, nlevels))
        assert f.read() == b''
    return out


def rows_from_visiting_order(n, src, dst, w, row_begin, row_end, hub_edges):
    """The row plan restated: the owned rows in the order the reference's loop first trains them, each with its firing edges in file order; a neighbour
    that the loop has trained before the row (an owned row first met earlier) is read from X_new (bit 31) and puts the row one level above it; inside
    a level the hub rows first, everything else in visiting order."""
    src = np.asarray(src, np.int64); dst = np.asarray(dst, np.int64)
    w = np.ones(len(src), np.float32) if w is None else np.asarray(w, np.float32)
    own = np.flatnonzero((dst > src) & (src >= row_begin) & (src < row_end))
    order, first_at = np.unique(src[own], return_index=True)
    order = order[np.argsort(first_at, kind='stable')]                       # rows by first visit
    pos = np.full(n, -1, np.int64); pos[order] = np.arange(len(order))
    by_row = own[np.argsort(pos[src[own]], kind='stable')]                   # a row's edges stay in file order
    deg = np.bincount(pos[src[own]], minlength=len(order))
    off = np.concatenate([[0], np.cumsum(deg)])
    col, wt = dst[by_row], w[by_row]
    new = (pos[col] >= 0) & (pos[col] < np.repeat(np.arange(len(order)), deg))
    level = np.zeros(len(order), np.int64)
    for r in range(len(order)):
        q = np.arange(off[r], off[r + 1])[new[off[r]:off[r + 1]]]
        level[r] = level[pos[col[q]]].max() + 1 if q.size else 0
    hub = (deg >= hub_edges) if hub_edges > 0 else np.zeros(len(order), bool)
    perm = np.lexsort((np.arange(len(order)), ~hub, level))                  # by level, hubs first, then visiting order
    nlevels = int(level.max()) + 1 if len(order) else 0
    edges = np.concatenate([np.arange(off[r], off[r + 1]) for r in perm]).astype(np.int64) if len(order) else np.zeros(0, np.int64)
    return dict(kind=0, rows=order[perm].astype(np.int32), ptr=np.concatenate([[0], np.cumsum(deg[perm])]).astype(np.int64),
                col=(col[edges] | (new[edges].astype(np.int64) << 31)).astype(np.uint32), w=wt[edges],
                level_off=np.concatenate([[0], np.cumsum(np.bincount(level, minlength=nlevels))]).astype(np.int64),
                level_hubs=np.bincount(level[hub], minlength=nlevels).astype(np.int64),
                level_maxlen=np.array([deg[(level == l) & ~hub].max(initial=0) for l in range(nlevels)], np.int64))


def scrambled_power_law(n, m, seed):
    """grouped by source, the sources first met in a scrambled order (multi-level), low ids with many more edges than high ones"""
    rs = np.random.RandomState(seed)
    src = np.minimum(rs.randint(0, n, m), rs.randint(0, n, m)).astype(np.int32); dst = rs.randint(0, n, m).astype(np.int32)
    by = np.argsort(rs.permutation(n)[src], kind='stable')
    return n, src[by], dst[by], (0.5 + rs.randint(0, 1000, m) / 8.0).astype(np.float32)[by]


def test_row_plans_equal_the_reference_visiting_order(driver, tmp_path, karate, sbm1024):
    kn, ks, kd, kw, _ = edge_arrays(karate)
    sn, ss, sd, sw, _ = edge_arrays(sbm1024)
    pn, ps, pd, pw = scrambled_power_law(4000, 12000, 9)
    cases = {
        'karate': (kn, ks, kd, kw, 0, kn, 1024),                   # node insertion order 0,31,21,19,..: several levels
        'karate_hubs': (kn, ks, kd, None, 0, kn, 3),               # most rows are hub rows
        'sbm1024': (sn, ss, sd, sw, 0, sn, 1024),
        'sbm1024_row_range': (sn, ss, sd, sw, 300, 811, 1024),     # a range strictly inside [0, n): neighbours outside it are read from X_old
        'power_law_hub8': (pn, ps, pd, pw, 0, pn, 8),
        'power_law_no_hubs': (pn, ps, pd, pw, 0, pn, 0),
        'self_loops': (8, [0, 0, 3, 1, 1, 2, 2, 5, 7, 4, 6, 6], [0, 3, 0, 1, 2, 1, 5, 5, 2, 6, 4, 7], None, 0, 8, 1024),
        'empty': (5, [], [], None, 0, 5, 1024),
    }
    for name, (n, src, dst, w, rb, r1, hub) in cases.items():
        assert row_schedule_represents(src, dst), name
        got = driver_rows(driver, tmp_path, n, src, dst, w, rb, r1, hub)
        want = rows_from_visiting_order(n, src, dst, w, rb, r1, hub)
        assert got.keys() == want.keys(), name
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k)
    want = rows_from_visiting_order(kn, ks, kd, kw, 0, kn, 1024)
    assert len(want['level_off']) > 2                                           # karate is multi-level ...
    want = rows_from_visiting_order(pn, ps, pd, pw, 0, pn, 8)
    assert (want['level_hubs'] > 0).any() and (want['level_hubs'] == 0).any()   # ... and the power law has levels with and without hub rows


def test_refusals_name_the_first_offending_edge(driver, tmp_path):
    """(1,2),(0,1),(1,3): edge 1 reads row 1 between its two updates (positions 0..2); an endpoint out of range is reported before that"""
    assert not row_schedule_represents([1, 0, 1], [2, 1, 3])
    assert driver_rows(driver, tmp_path, 4, [1, 0, 1], [2, 1, 3], None, 0, 4, 1024) == dict(kind=2, edge=1, first=0, last=2)
    assert driver_rows(driver, tmp_path, 4, [1, 0, 1], [2, 1, 4], None, 0, 4, 1024) == dict(kind=1, edge=2, first=-1, last=-1)
