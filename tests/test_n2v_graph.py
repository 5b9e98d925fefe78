"""CPU tests of node2vec's device-free graph set-up (gem_amd/csrc/n2v_graph.hip: prepare_n2v_graph, the renaming of the binary-layout unigram
table) and of sgns_knobs_from_env (gem_amd/csrc/sgns_plan.hip), as plain C++ behind scripts/asan/n2v_graph_driver.cpp: no HIP, no device.
Integer results must be exact and weights bit for bit.  The refusals are also taken through the library: gemhip_n2v_create makes them before
its first HIP call, and words them as tests/golden/n2v_create_refusals.txt records from the library before the set-up moved out of n2v.hip."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
from conftest import golden_path
from gem_amd import _hip, build
from test_oracle_n2v import small_graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, N_OUT_OF_RANGE, BAD_ARRAYS, ROW_PTR_FIRST, ROW_PTR_LAST, ROW_PTR_NOT_MONOTONE, COLUMN_OUT_OF_RANGE, NON_POSITIVE_WEIGHT = range(8)    # N2vGraphError::Kind
ALIAS_HUB_DEG = 2048


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    d = tmp_path_factory.mktemp('n2v_graph')
    exe = str(d / 'n2v_graph_driver')
    csrc = os.path.join(ROOT, 'gem_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(csrc, 'n2v_graph.hip'), os.path.join(csrc, 'sgns_plan.hip'),
                           os.path.join(ROOT, 'scripts', 'asan', 'n2v_graph_driver.cpp'), '-o', exe])

    class Driver:
        def graph(self, n, nnz, row_ptr, col, w, hub_deg=ALIAS_HUB_DEG):
            """prepare_n2v_graph: (kind, index, column) of a refusal, or a dict of N2vGraph's fields."""
            rp = np.zeros(0, np.int64) if row_ptr is None else np.ascontiguousarray(row_ptr, np.int64)
            c = np.zeros(0, np.int32) if col is None else np.ascontiguousarray(col, np.int32)
            with open(d / 'in', 'wb') as f:
                np.array([n, nnz, hub_deg, w is not None, len(rp), len(c)], np.int64).tofile(f)
                rp.tofile(f); c.tofile(f)
                if w is not None:
                    np.ascontiguousarray(w, np.float32).tofile(f)
            subprocess.check_call([exe, 'graph', str(d / 'in'), str(d / 'out')])
            raw = open(d / 'out', 'rb').read()
            kind, index, column = np.frombuffer(raw, np.int64, 3)
            if kind != NONE:
                return int(kind), int(index), int(column)
            uniform, nstart, nhub, nw = (int(v) for v in np.frombuffer(raw, np.int64, 4, 24))
            at, out = 56, {'uniform': bool(uniform)}
            for name, dtype, count in (('col', np.int32, len(c)), ('w', np.float32, nw), ('start', np.int32, nstart), ('hub_rows', np.int32, nhub),
                                       ('hub_off', np.int64, (len(raw) - 56 - 4 * (len(c) + nw + nstart + nhub)) // 8)):
                out[name] = np.frombuffer(raw, dtype, count, at); at += count * np.dtype(dtype).itemsize
            assert at == len(raw)
            return out

        def rename(self, n, back, U, K):
            with open(d / 'in', 'wb') as f:
                np.array([n, len(back)], np.int64).tofile(f)
                np.ascontiguousarray(back, np.int32).tofile(f); np.ascontiguousarray(U, np.float32).tofile(f); np.ascontiguousarray(K, np.int32).tofile(f)
            subprocess.check_call([exe, 'rename', str(d / 'in'), str(d / 'out')])
            raw = open(d / 'out', 'rb').read()
            return np.frombuffer(raw, np.float32, len(back)), np.frombuffer(raw, np.int32, len(back), 4 * len(back))

        def knobs(self, **env):
            out = subprocess.check_output([exe, 'knobs'] + ['GEMHIP_SGNS_%s=%s' % kv for kv in env.items()])
            return dict(zip(KNOBS, (int(v) for v in out.split())))
    drv = Driver()
    drv.exe = exe
    return drv


def test_self_checks_pass(driver):
    run = subprocess.run([driver.exe, 'self'], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-3000:]


def unsorted_csr(n, src, dst, w, seed=0):
    """The edge list as a CSR whose rows keep a shuffled edge order: (row_ptr, col, w) as a caller may hand them to gemhip_n2v_create."""
    perm = np.random.RandomState(seed).permutation(len(src))
    perm = perm[np.argsort(np.asarray(src)[perm], kind='stable')]
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    return row_ptr, np.asarray(dst, np.int32)[perm], None if w is None else np.asarray(w, np.float32)[perm]


def check_against_oracle(driver, n, src, dst, w, hub_deg=ALIAS_HUB_DEG, uniform=None):
    row_ptr, col, ww = unsorted_csr(n, src, dst, w)
    g = driver.graph(n, len(col), row_ptr, col, ww, hub_deg)
    assert isinstance(g, dict), g
    # the oracle sorts the same edge list by (row, column), ties in list order: put the list in the CSR's order first
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    rp, cs, ws = oracle.sorted_csr(n, rows, col, ww)
    assert np.array_equal(rp, row_ptr) and np.array_equal(g['col'], cs)
    assert (g['w'].size == 0) if w is None else (g['w'].tobytes() == ws.tobytes())
    assert np.array_equal(g['start'], oracle.start_nodes(rp, cs))
    if uniform is not None:
        assert g['uniform'] == uniform
    deg = np.diff(row_ptr)
    hubs = np.flatnonzero(deg >= hub_deg)
    if g['uniform']:
        assert g['hub_rows'].size == 0 and g['hub_off'].size == 0
    else:
        assert np.array_equal(g['hub_rows'], hubs) and np.array_equal(g['hub_off'], np.concatenate([[0], np.cumsum(deg[hubs])]))
    return g


@pytest.mark.parametrize('weighted', [False, True])
def test_rows_are_sorted_with_their_weights_following(driver, weighted):
    n, src, dst, w = small_graph(weighted, seed=3, n=200, m=3000)
    row_ptr, col, _ = unsorted_csr(n, src, dst, w)
    assert any(np.any(np.diff(col[a:b]) < 0) for a, b in zip(row_ptr[:-1], row_ptr[1:]))            # (the rows do arrive unsorted)
    check_against_oracle(driver, n, src, dst, w, uniform=not weighted)


def test_a_repeated_column_keeps_the_order_of_its_weights(driver):
    """The sort is stable: two edges of one row to the same column keep their order, which is the order n2v_alias_rows_kernel sees their weights in."""
    row_ptr = np.array([0, 5, 5, 6], np.int64); col = np.array([2, 1, 2, 1, 0, 0], np.int32); w = np.array([1, 2, 3, 4, 5, 7], np.float32)
    g = driver.graph(3, 6, row_ptr, col, w)
    assert list(g['col']) == [0, 1, 1, 2, 2, 0] and list(g['w']) == [5, 2, 4, 1, 3, 7] and not g['uniform']
    assert list(g['start']) == [0, 1, 2]


def test_isolated_ids_and_a_sink(driver):
    """The 40-node graph of test_isolated_nodes_never_start_a_walk: a sink starts walks (it occurs in the edge list), an isolated id does not."""
    src = np.array([0, 1, 2, 5, 5, 9, 30], np.int32); dst = np.array([1, 2, 0, 9, 2, 5, 31], np.int32)
    g = check_against_oracle(driver, 40, src, dst, None, uniform=True)
    assert list(g['start']) == [0, 1, 2, 5, 9, 30, 31]


def test_hub_rows_and_their_offsets(driver):
    """Two rows of at least 8 neighbours at hub_deg = 8: hub_rows names them, hub_off is the prefix sum of their degrees."""
    src = np.concatenate([np.full(9, 3), np.full(7, 5), np.full(8, 11), [0, 1]]).astype(np.int32)
    dst = np.concatenate([np.arange(9)[::-1] + 4, np.arange(7), np.arange(8)[::-1], [3, 11]]).astype(np.int32)
    w = (1.0 + np.arange(len(src)) % 5).astype(np.float32)
    g = check_against_oracle(driver, 16, src, dst, w, hub_deg=8, uniform=False)
    assert list(g['hub_rows']) == [3, 11] and list(g['hub_off']) == [0, 9, 17]
    g = check_against_oracle(driver, 16, src, dst, w)                     # ... and none at the library's threshold
    assert g['hub_rows'].size == 0 and list(g['hub_off']) == [0]


def test_weights_that_differ_between_rows_only_are_uniform(driver):
    n, src, dst, _ = small_graph(False, seed=3, n=200, m=3000)
    w = (0.5 + src % 7).astype(np.float32)
    g = check_against_oracle(driver, n, src, dst, w, hub_deg=8, uniform=True)
    assert g['w'].size == len(src)


# ---- refusals: (what, n, nnz, row_ptr, col, w, kind, index of the first offender), on a 3-node path graph; tests/golden/n2v_create_refusals.txt holds
# the library's text for each, in this order
PATH_RP, PATH_COL = [0, 1, 3, 4], [1, 0, 2, 1]
REFUSALS = (('n out of range', 0, 4, PATH_RP, PATH_COL, None, N_OUT_OF_RANGE, 0),
            ('row_ptr[0] != 0', 3, 4, [1, 1, 3, 4], PATH_COL, None, ROW_PTR_FIRST, 0),
            ('row_ptr[n] != nnz', 3, 4, [0, 1, 3, 3], PATH_COL, None, ROW_PTR_LAST, 3),
            ('row_ptr not monotone', 3, 4, [0, 3, 1, 4], PATH_COL, None, ROW_PTR_NOT_MONOTONE, 1),
            ('column outside [0, n)', 3, 4, PATH_RP, [1, 0, 3, -1], None, COLUMN_OUT_OF_RANGE, 2),
            ('non-positive weight', 3, 4, PATH_RP, PATH_COL, [1.0, 2.0, 0.0, -1.0], NON_POSITIVE_WEIGHT, 2))


@pytest.mark.parametrize('case', REFUSALS, ids=[c[0] for c in REFUSALS])
def test_refusal_names_the_first_offender(driver, case):
    what, n, nnz, rp, col, w, kind, index = case
    got = driver.graph(n, nnz, rp, col, w)
    assert got[:2] == (kind, index), got
    if kind == COLUMN_OUT_OF_RANGE:
        assert got[2] == 3


def test_more_refusals(driver):
    assert driver.graph(2 ** 31 - 1, 4, PATH_RP, PATH_COL, None)[0] == N_OUT_OF_RANGE
    assert driver.graph(3, 4, None, PATH_COL, None)[0] == BAD_ARRAYS and driver.graph(3, 4, PATH_RP, None, None)[0] == BAD_ARRAYS
    assert driver.graph(3, -1, PATH_RP, PATH_COL, None)[0] == BAD_ARRAYS
    assert driver.graph(3, 4, PATH_RP, PATH_COL, [1, 1, float('nan'), 1])[:2] == (NON_POSITIVE_WEIGHT, 2)


def library_refusal(case):
    """gemhip_n2v_create on the case: (return code, handle, gemhip_last_error())."""
    what, n, nnz, rp, col, w, kind, index = case
    L = _hip.lib()
    rp, col, w = np.array(rp, np.int64), np.array(col, np.int32), None if w is None else np.array(w, np.float32)
    h = C.c_void_p()
    rc = L.gemhip_n2v_create(n, nnz, _hip.ptr(rp, C.c_int64), _hip.ptr(col, C.c_int32), _hip.ptr(w, C.c_float), C.byref(h))
    return rc, h.value, L.gemhip_last_error().decode()


def test_the_library_words_every_refusal_as_before():
    """The same six refusals through gemhip_n2v_create: they precede its first HIP call, so this runs without a GPU."""
    want = open(golden_path('n2v_create_refusals.txt')).read().splitlines()
    assert len(want) == len(REFUSALS)
    for case, text in zip(REFUSALS, want):
        rc, h, msg = library_refusal(case)
        assert rc == _hip.E_INVALID and not h, case[0]
        assert msg == text, case[0]


def test_renaming_of_the_binary_layout_table(driver, sbm1024):
    """UT_out / KT_out of gemhip_n2v_build_unigram_vocab_order: the table by node becomes the table in renamed indices -- on the SBM-1024 counts of
    one round of walks, a third of the nodes never occurring, and a random first-appearance order."""
    from gem_amd.graph import edge_arrays
    n, src, dst, _, _ = edge_arrays(sbm1024)
    rp, cs, _ = oracle.sorted_csr(n, src, dst, None)
    counts = oracle.n2v_vocab(n, oracle.n2v_walks(rp, cs, None, None, 1.0, 1.0, 1, 40, 3, 11))
    counts[::3] = 0
    rs = np.random.RandomState(5)
    back = rs.permutation(np.flatnonzero(counts > 0)).astype(np.int32)                    # renamed id -> node
    U = rs.rand(n).astype(np.float32)
    K = back[rs.randint(0, len(back), n)].astype(np.int32)                                 # an alias is a node that occurs
    UT, KT = driver.rename(n, back, U, K)
    renamed = np.zeros(n, np.int32); renamed[back] = np.arange(len(back))
    assert UT.tobytes() == U[back].tobytes() and np.array_equal(KT, renamed[K[back]])


# ---- GEMHIP_SGNS_* -> SgnsKnobs, as gemhip_n2v_create has always clamped them: (variable, knob, default, {value: knob}) below, inside and above the range
KNOBS = ('max_waves', 'cache_radius', 'cache_delta', 'prefetch', 'reload', 'hot_count', 'local_hot', 'fresh', 'neg_count')
KNOB_TABLE = (('MAX_WAVES', 'max_waves', 0, {-3: 0, 0: 0, 512: 512, 2 ** 31 - 1: 2 ** 31 - 1}),          # max(0, v)
              ('CACHE_R', 'cache_radius', -1, {-7: -1, -1: -1, 0: 0, 10: 10, 31: 31, 32: 31, 1000: 31}),  # clamp to [-1, 31]
              ('CACHE_DELTA', 'cache_delta', -1, {-2: -1, -1: -1, 0: 0, 1: 1, 2: 1}),                     # clamp to [-1, 1]
              ('PREFETCH', 'prefetch', 2, {-1: 1, 0: 1, 1: 1, 2: 2, 3: 2}),                               # clamp to [1, 2]
              ('RELOAD', 'reload', 1, {-1: 1, 0: 0, 1: 1, 5: 1}),                                         # v != 0
              ('HOT_COUNT', 'hot_count', -1, {-9: -1, -1: -1, 0: 0, 50: 50}),                             # max(-1, v)
              ('LOCAL_HOT', 'local_hot', 8, {-1: 0, 0: 0, 8: 8, 100: 100}),                               # max(0, v)
              ('FRESH', 'fresh', 0, {-1: 7, 0: 0, 5: 5, 7: 7, 8: 0, 13: 5}),                              # v & 7
              ('NEG_COUNT', 'neg_count', 0, {-4: 0, 0: 0, 30: 30}))                                       # max(0, v)


def test_knobs_without_environment_are_the_defaults(driver):
    assert driver.knobs() == {knob: default for _, knob, default, _ in KNOB_TABLE}
    assert driver.knobs(UNKNOWN=5, MAX_WAVES='') == {knob: default for _, knob, default, _ in KNOB_TABLE}      # ('' reads as 0, the default)


@pytest.mark.parametrize('var,knob,default,values', KNOB_TABLE, ids=[k[0] for k in KNOB_TABLE])
def test_knob_clamps(driver, var, knob, default, values):
    for value, want in values.items():
        got = driver.knobs(**{var: value})
        assert got == {**{k: d for _, k, d, _ in KNOB_TABLE}, knob: want}, (var, value)
    assert driver.knobs(**{var: 'junk'})[knob] == {'MAX_WAVES': 0, 'CACHE_R': 0, 'CACHE_DELTA': 0, 'PREFETCH': 1, 'RELOAD': 0, 'HOT_COUNT': 0, 'LOCAL_HOT': 0,
                                                  'FRESH': 0, 'NEG_COUNT': 0}[var]       # atoi of a non-number is 0, then the clamp
