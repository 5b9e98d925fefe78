"""CPU tier of the neighbourhood link-prediction baselines (gem_amd/csrc/nbr_host.hip, gem_amd/evaluation/link_heuristics.py): the
restatements of tests/nbr_refs.py against networkx, the host ingest against the restated CSR, the weight rule against CPython's math.log,
the planner's counts, every refusal with its message, the device entries without a device, and the golden file against its generator."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

import nbr_refs as NB
import rank_refs as R
from conftest import ROOT, golden_path
from gem_amd import _hip
from gem_amd.evaluation import link_classification as LC
from gem_amd.evaluation import link_heuristics as LH
from gem_amd.graph import EdgeListGraph

sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_link_baselines as MG  # noqa: E402


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def graph_host(n, src, dst):
    src = i32(src); dst = i32(dst)
    row_ptr = np.full(n + 1, -1, np.int64); col = np.full(2 * len(src) + 1, -1, np.int32); deg = np.full(n, -1, np.int32)
    rc = _hip.lib().gemhip_nbr_graph_host(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32),
                                          _hip.ptr(deg, C.c_int32))
    return rc, row_ptr, col, deg


def plan_host(deg, st, ed, m=None):
    deg = i32(deg); st = i32(st); ed = i32(ed)
    counts = np.full(6, -1, np.int64)
    rc = _hip.lib().gemhip_nbr_plan_host(len(deg), _hip.ptr(deg, C.c_int32), len(st) if m is None else m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32),
                                         _hip.ptr(counts, C.c_int64))
    return rc, counts


def last_error():
    return _hip.lib().gemhip_last_error().decode()


@pytest.fixture(scope='module')
def fixture_scores():
    """The fixture's train graph, its test pairs, the restated scores and networkx's, computed once."""
    train, _, pairs = R.fixture_pairs()
    st, ed, y = pairs['test']
    A = NB.simple_csr(train.n, train.src, train.dst)
    return train, A, st, ed, y, NB.scores(A, st, ed), MG.networkx_scores(MG.train_nx_graph(train), st, ed)


def test_constants_are_the_ones_the_restatements_use():
    assert LH.constants() == {'lanes_per_narrow_group': NB.LANES, 'narrow': NB.NARROW, 'chunk': NB.CHUNK}
    assert LH.HEURISTICS == NB.HEURISTICS == MG.HEURISTICS


def test_restatements_against_networkx_on_the_fixture_pairs(fixture_scores):
    _, A, st, ed, _, ref, nxs = fixture_scores
    for name in ('cn', 'jaccard', 'pa'):
        assert np.array_equal(ref[name].astype(np.float64), nxs[name]), name
    assert ref['cn'].max() >= 3 and (ref['cn'] == 0).any()
    w_aa, w_ra = NB.weight_tables(NB.degrees(A))
    for name, table in (('aa', w_aa), ('ra', w_ra)):
        exact = NB.fsum_scores(table, A, st, ed)
        bound = NB.sum_bound(ref['cn'], exact)
        for got in (ref[name], nxs[name]):
            assert np.all(np.abs(got - exact) <= bound), name


def test_host_ingest_against_the_restated_csr(fixture_scores):
    train = fixture_scores[0]
    n, hs, hd = NB.hand_graph()
    cases = [(n, hs, hd),                                                         # self-loop, repeats, one-sided arcs, an isolated node
             (5, [], []),                                                         # an empty list
             (7, [6, 6, 2], [2, 2, 6]),                                           # isolated nodes 0, 1, 3, 4, 5
             (4, [1, 2], [1, 2]),                                                 # self-loops only
             (train.n, train.src, train.dst)]
    n2, s2, d2, _, _ = NB.two_hub_graph(NB.NARROW + 1, 4 * NB.NARROW + 9, 11)
    cases.append((n2, s2, d2))
    for n, src, dst in cases:
        rc, row_ptr, col, deg = graph_host(n, src, dst)
        assert rc == 0, last_error()
        A = NB.simple_csr(n, src, dst)
        assert np.array_equal(row_ptr, A.indptr) and np.array_equal(col[:A.nnz], A.indices) and np.array_equal(deg, NB.degrees(A))
        assert np.all(col[A.nnz:] == -1)                                          # nothing written past the stored neighbours


def test_weight_rule_against_cpython_log():
    """w_aa[k] = 1.0 / std::log((double)k) against 1.0 / math.log(k) for every k in 2 .. 2^22 (both are the machine's libm), and w_ra[k] =
    1.0 / k.  The condition is <= 2 ulp; observed: equal everywhere (0 ulp)."""
    top = 1 << 22
    deg = np.arange(top + 1, dtype=np.int32)
    w = np.zeros(top + 1)
    L = _hip.lib()
    _hip.check(L.gemhip_nbr_weights_host(top + 1, _hip.ptr(deg, C.c_int32), 0, _hip.ptr(w, C.c_double)))
    want = np.array([0.0, 0.0] + [1.0 / math.log(k) for k in range(2, top + 1)])
    ulps = np.abs(w.view(np.int64) - want.view(np.int64))
    print('largest deviation of w_aa from 1.0 / math.log(k), k = 2 .. 2^22: %d ulp' % ulps.max())
    assert ulps.max() <= 2
    _hip.check(L.gemhip_nbr_weights_host(top + 1, _hip.ptr(deg, C.c_int32), 1, _hip.ptr(w, C.c_double)))
    assert w[0] == 0.0 and np.array_equal(w[1:], 1.0 / deg[1:].astype(np.float64))
    assert L.gemhip_nbr_weights_host(3, _hip.ptr(deg, C.c_int32), 2, _hip.ptr(w, C.c_double)) == _hip.E_INVALID


def test_plan_counts_for_degrees_straddling_narrow_and_chunk():
    N, K = NB.NARROW, NB.CHUNK
    las = [1, N - 1, N, N + 1, K - 1, K, K + 1, K + N, K + N + 1, 2 * K, 2 * K + 3, 5 * K + N]
    deg = np.array(las + [6 * K, 0], np.int32)                                    # node len(las): longer than every la; the last node: degree 0
    big, none = len(las), len(las) + 1
    deg = np.concatenate([deg, np.zeros(6 * K + 1 - len(deg), np.int32)])          # plan_host wants deg < n
    st = np.arange(len(las)); ed = np.full(len(las), big)
    for a, b in ((st, ed), (ed, st), (np.concatenate([st, st[::-1]]), np.concatenate([ed, ed[::-1]]))):
        rc, counts = plan_host(deg, a, b)
        assert rc == 0, last_error()
        assert tuple(counts[:4]) == NB.plan_counts(deg, a, b)
        assert counts[4] == K and counts[5] == 0
    for q, la in enumerate(las):                                                   # one pair at a time: which class each length lands in
        rc, counts = plan_host(deg, [q], [big])
        pieces = -(-la // K)
        tail = la - (pieces - 1) * K
        narrow = int(tail <= N)
        assert tuple(counts[:6]) == (narrow, pieces - narrow, int(la > K), pieces if la > K else 0, min(la, K), 0), la
    rc, counts = plan_host(deg, [none, 0, big], [big, none, none])                 # la == 0: no item
    assert rc == 0 and tuple(counts[:6]) == (0, 0, 0, 0, 0, 3)
    rc, counts = plan_host(deg, [1, 2], [2, 1])                                    # equal and unequal lengths: one item per pair
    assert rc == 0 and tuple(counts[:4]) == (2, 0, 0, 0)


def test_every_refusal_with_its_message():
    L = _hip.lib()
    h = C.c_void_p()
    good = i32([0, 1, 2])

    def create(n, src, dst, m=None):
        src = i32(src); dst = i32(dst)
        rc = L.gemhip_nbr_create(n, len(src) if m is None else m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), C.byref(h))
        assert not h.value or rc == 0
        return rc

    for who, call in (('nbr_create', create), ('nbr_graph_host', lambda n, s, d: graph_host(n, s, d)[0])):
        assert call(0, [], []) == _hip.E_INVALID and last_error() == '%s: n = 0 (need n >= 1)' % who
        assert call(4, [0, 4, 9], [1, 1, 1]) == _hip.E_INVALID and last_error() == '%s: arc 1 = (4,1) outside [0,4)' % who
        assert call(4, [0, 1, 2], [1, -1, 7]) == _hip.E_INVALID and last_error() == '%s: arc 1 = (1,-1) outside [0,4)' % who
    assert create(1 << 31, [], []) == _hip.E_UNSUPPORTED and last_error() == 'nbr_create: n = 2147483648: must be below 2^31'
    assert create(4, [], [], m=-1) == _hip.E_INVALID and last_error() == 'nbr_create: m = -1 arcs (need m >= 0)'
    assert L.gemhip_nbr_create(4, 2, None, None, C.byref(h)) == _hip.E_INVALID and last_error() == 'nbr_create: NULL arc arrays'

    deg = [1, 1, 2, 0, 0]
    for st, ed, rc_want, msg in (([0, 5, 1], [1, 1, 1], _hip.E_INVALID, 'pair 1 = (5,1) outside [0,5)'),                     # a later pair is a self-pair
                                 ([0, 1], [1, -1], _hip.E_INVALID, 'pair 1 = (1,-1) outside [0,5)'),
                                 ([0, 2, 9], [1, 2, 0], _hip.E_INVALID, 'pair 1 = (2,2): st == ed (the scores are defined for two different nodes)'),
                                 ([], [], _hip.E_INVALID, 'm = 0 pairs (need m >= 1)')):
        rc, counts = plan_host(deg, st, ed)
        assert rc == rc_want and last_error() == 'nbr_plan_host: ' + msg
        assert np.all(counts == -1)                                                # nothing was written
    rc, _ = plan_host(deg, good, good, m=1 << 31)
    assert rc == _hip.E_UNSUPPORTED and last_error() == 'nbr_plan_host: m = 2147483648: must be below 2^31'
    rc, _ = plan_host([1, 5, 0], [0], [1])
    assert rc == _hip.E_INVALID and last_error() == 'nbr_plan_host: deg[1] = 5 outside [0,3)'
    assert L.gemhip_nbr_scores(None, 1, _hip.ptr(good, C.c_int32), _hip.ptr(good, C.c_int32), 1, None, None, None, None, None) == _hip.E_INVALID
    assert last_error() == 'nbr_scores: NULL handle'
    with pytest.raises(ValueError, match="heuristic 'katz': one of cn, jaccard, aa, ra, pa"):
        LH._names(('cn', 'katz'))
    with pytest.raises(ValueError, match="operator 'cosine'"):                     # the operators' own message is unchanged
        LC._op_id('cosine')


def test_unknown_op_lists_the_new_names_after_the_old_text():
    pairs = {'test': (i32([0]), i32([1]), np.ones(1, np.uint8)), 'train': (i32([0]), i32([1]), np.ones(1, np.uint8))}
    with pytest.raises(ValueError) as e:
        LC._score_pairs(None, pairs, 'katz', 1.0, None, None, None)
    old = "op = 'katz': one of average, hadamard, l1, l2, 'dot', 'method'"
    assert str(e.value).startswith(old) and str(e.value).endswith('cn, jaccard, aa, ra, pa')
    with pytest.raises(ValueError, match="op='aa' needs train_graph"):
        LC._score_pairs(None, pairs, 'aa', 1.0, None, None, None)
    assert LC.OPERATORS == {'average': 0, 'hadamard': 1, 'l1': 2, 'l2': 3} and LC.FEATURE_OPS == ('average', 'hadamard', 'l1', 'l2')


def test_every_device_entry_raises_without_a_device():
    if _hip.device_count() > 0:
        pytest.skip('GPU present')
    g = EdgeListGraph(4, [0, 1, 2], [1, 2, 3])
    for call in (lambda: LH.NeighbourScorer(g), lambda: LH.evaluate_link_heuristics(g, g), lambda: LH.evaluateStaticLinkHeuristics(g),
                 lambda: LH.expLinkHeuristics(g, 1), lambda: LC.evaluate_link_classification(g, g, None, op='cn')):
        with pytest.raises(_hip.GemHipError):
            call()
    h = C.c_void_p()
    src = i32([0, 1]); dst = i32([1, 2])
    assert _hip.lib().gemhip_nbr_create(3, 2, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), C.byref(h)) == _hip.E_HIP and not h.value


def test_golden_file_regenerates_from_its_generator(fixture_scores):
    _, _, _, _, y, ref, nxs = fixture_scores
    stored = json.load(open(golden_path('link_baselines_ref.json')))
    fresh = MG.report()
    assert set(stored['heuristics']) == set(LH.HEURISTICS)
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        assert stored[k] == fresh[k]
    for name in LH.HEURISTICS:
        a, b = stored['heuristics'][name], fresh['heuristics'][name]
        assert set(a) == set(b)
        for k in a:
            if k in ('n_thresholds', 'near'):
                assert a[k] == b[k], (name, k)
            elif k != 'sklearn_vs_exact':                                           # (sklearn's own rounding may move with its version)
                assert abs(a[k] - b[k]) <= 1e-12 * max(abs(a[k]), 1e-300), (name, k)
        ex = R.exact_scores(nxs[name], y)
        assert a['n_thresholds'] == ex['T'] and abs(a['auc'] - float(ex['auc'])) <= 1e-12 and abs(a['ap'] - float(ex['ap'])) <= 1e-12
