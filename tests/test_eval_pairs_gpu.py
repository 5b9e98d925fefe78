"""GPU: the evaluator handle of gem_amd/csrc/eval.hip -- pair scores and edge hits against fp64 numpy, evaluate_reconstruction_gpu against
tests/golden/eval_pairs_ref.json (the reference's evaluate_graph_reconstruction.py:8-46, evaluation_util.py:5-36, metrics.py:6-46 on an
explicit pair list), and the distance-kernel AP of Laplacian Eigenmaps / LLE against average_precision_rows."""
import ctypes as C

import numpy as np
import pytest

from gem_amd import _hip
from gem_amd.embedding.lap import LaplacianEigenmaps
from gem_amd.embedding.lle import LocallyLinearEmbedding
from gem_amd.evaluation import reconstruction as gr
from gem_amd.graph import EdgeListGraph, edge_arrays, to_csr
from conftest import golden_path
from test_eval_pairs import CASES, REF, embedding_of, model_of, weighted_karate

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ the pair kernel against fp64 numpy
N, NPAIRS = 300, 1003


class Handle(object):
    def __init__(self, n, da, ld, A, B, kind, row_ptr, col):
        self.h = C.c_void_p()
        _hip.check(_hip.lib().gemhip_eval_create(n, da, ld, _hip.ptr(A, C.c_float), _hip.ptr(B, C.c_float), kind, _hip.ptr(row_ptr, C.c_int64),
                                                 _hip.ptr(col, C.c_int32), C.byref(self.h)))

    def pairs(self, st, ed, want_hit=True):
        score = np.full(len(st), np.nan); hit = np.full(len(st), 7, np.uint8) if want_hit else None
        _hip.check(_hip.lib().gemhip_eval_pairs(self.h, len(st), _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(score, C.c_double),
                                                _hip.ptr(hit, C.c_uint8)))
        return score, hit

    def ap(self, nodes, undirected):
        out = np.zeros(len(nodes))
        _hip.check(_hip.lib().gemhip_eval_ap(self.h, int(undirected), len(nodes), _hip.ptr(nodes, C.c_int32), _hip.ptr(out, C.c_double)))
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _hip.check(_hip.lib().gemhip_eval_destroy(self.h))


@pytest.fixture(scope='module')
def pair_problem():
    """A random directed graph on 300 nodes in which row 3 holds every column but four and row 4 is empty; 1003 pairs (no multiple of a
    group, a wavefront or a workgroup) with self-pairs, both ends of the long row and pairs out of the empty row."""
    rng = np.random.RandomState(11)
    src = rng.randint(0, N, 2500); dst = rng.randint(0, N, 2500)
    keep = (src != 4) & (src != 3)
    long_row = np.setdiff1d(np.arange(N), [3, 17, 150, 299])
    src = np.concatenate([src[keep], np.full(len(long_row), 3)]); dst = np.concatenate([dst[keep], long_row])
    key = np.unique(src.astype(np.int64) * N + dst)
    src, dst = (key // N).astype(np.int32), (key % N).astype(np.int32)
    row_ptr, col, _ = to_csr(N, src, dst, None, sort_cols=True)
    adj = np.zeros((N, N), dtype=bool); adj[src, dst] = True
    st = rng.randint(0, N, NPAIRS).astype(np.int32); ed = rng.randint(0, N, NPAIRS).astype(np.int32)
    st[:8] = [3, 3, 3, 3, 4, 4, 9, 299]; ed[:8] = [0, 298, 17, 299, 0, 299, 9, 299]
    return row_ptr, col, adj, st, ed


@pytest.fixture(scope='module')
def wide_row_problem():
    """700 nodes: row 0 has 600 > 512 neighbours, row 1 none -- the binary search over a long and over an empty range.  Rows 0 and 1 are
    asked for every column, plus three random pairs (1403 in all)."""
    n = 700
    rng = np.random.RandomState(12)
    nb = rng.choice(np.arange(1, n), 600, replace=False)
    src = np.concatenate([np.zeros(600, np.int64), rng.randint(2, n, 900)]); dst = np.concatenate([nb, rng.randint(0, n, 900)])
    key = np.unique(src * n + dst)
    src, dst = (key // n).astype(np.int32), (key % n).astype(np.int32)
    row_ptr, col, _ = to_csr(n, src, dst, None, sort_cols=True)
    assert row_ptr[1] - row_ptr[0] == 600 and row_ptr[2] == row_ptr[1]
    adj = np.zeros((n, n), dtype=bool); adj[src, dst] = True
    every = np.arange(n, dtype=np.int32)
    st = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32), rng.randint(0, n, 3).astype(np.int32)])
    ed = np.concatenate([every, every, rng.randint(0, n, 3).astype(np.int32)])
    return n, row_ptr, col, adj, st, ed


def operands(n, d, split, kind, pad, seed):
    """A, B as the handle takes them ([n][ld] float32, ld = da + pad) and their fp64 views [n][da]."""
    rng = np.random.RandomState(seed)
    da = d // 2 if split else d
    scale = 1.0 if kind == 0 else 0.7 / np.sqrt(da)                           # kind 1: squared distances of order 1, far from exp's underflow
    A = np.full((n, da + pad), np.float32(1e30)); A[:, :da] = (rng.randn(n, da) * scale).astype(np.float32)
    B = None
    if split:
        B = np.full((n, da + pad), np.float32(1e30)); B[:, :da] = rng.randn(n, da).astype(np.float32)
    return da, A, B


def numpy_scores(A, B, da, kind, st, ed):
    a = A[st, :da].astype(np.float64); b = (A if B is None else B)[ed, :da].astype(np.float64)
    if kind == 0:
        s = (a * b).sum(axis=1); mag = np.abs(a * b).sum(axis=1)
    else:
        s = np.exp(-np.linalg.norm(a - b, axis=1) ** 2); mag = None
    s[st == ed] = 0.0
    return s, mag


SHAPES = [(d, False, kind, 0) for d in (1, 2, 63, 64, 65, 128, 130, 512) for kind in (0, 1)] + \
         [(4, True, 0, 0), (130, True, 0, 0),                                  # HOPE: A = X[:, :k], B = X[:, k:]
          (63, False, 0, 1), (63, False, 1, 1), (130, False, 1, 2), (5, False, 0, 3), (509, False, 1, 3)]   # ld > da: 16-byte path with a masked tail


@pytest.mark.parametrize('d,split,kind,pad', SHAPES)
def test_pair_scores_and_hits_against_numpy(pair_problem, d, split, kind, pad):
    row_ptr, col, adj, st, ed = pair_problem
    da, A, B = operands(N, d, split, kind, pad, seed=d + 7 * kind)
    with Handle(N, da, da + pad, A, B, kind, row_ptr, col) as h:
        score, hit = h.pairs(st, ed)
        score2, hit2 = h.pairs(st, ed)
        only_score, none = h.pairs(st, ed, want_hit=False)
        _hip.check(_hip.lib().gemhip_eval_pairs(h.h, 0, None, None, None, None))                 # npairs = 0 is legal
    want, mag = numpy_scores(A, B, da, kind, st, ed)
    err = np.abs(score - want)
    if kind == 0:
        bound = 4 * da * 2.0 ** -53 * mag                          # fp64 summation in another order: (d - 1) u sum|a_k b_k| on either side
        print('kind 0 d=%d ld=%d: max |delta| / bound = %.3g' % (da, da + pad, (err[mag > 0] / bound[mag > 0]).max() if (mag > 0).any() else 0.0))
        assert np.all(err <= bound)
    else:
        print('kind 1 d=%d ld=%d: max relative error %.3g' % (da, da + pad, (err[want > 0] / want[want > 0]).max()))
        assert np.all(err <= 1e-13 * want)
    assert np.all(score[st == ed] == 0.0)
    assert np.array_equal(hit, adj[st, ed].astype(np.uint8))
    assert score.tobytes() == score2.tobytes() and hit.tobytes() == hit2.tobytes() and only_score.tobytes() == score.tobytes()


def test_edge_lookup_in_a_row_of_more_than_512_and_in_an_empty_row(wide_row_problem):
    n, row_ptr, col, adj, st, ed = wide_row_problem
    da, A, B = operands(n, 8, False, 0, 0, seed=1)
    with Handle(n, da, da, A, None, 0, row_ptr, col) as h:
        score, hit = h.pairs(st, ed)
    assert np.array_equal(hit, adj[st, ed].astype(np.uint8))
    assert hit[:n].sum() == 600 and hit[n:2 * n].sum() == 0


def test_handle_rejects_bad_input_with_messages(pair_problem):
    row_ptr, col, adj, st, ed = pair_problem
    da, A, B = operands(N, 4, False, 0, 0, seed=1)
    L = _hip.lib()
    h = C.c_void_p()
    assert L.gemhip_eval_create(N, 4, 4, _hip.ptr(A, C.c_float), None, 2, _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), C.byref(h)) == _hip.E_INVALID
    assert b'kind 2' in L.gemhip_last_error() and not h.value
    assert L.gemhip_eval_create(N, 513, 513, _hip.ptr(A, C.c_float), None, 0, _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), C.byref(h)) == _hip.E_INVALID
    unsorted = col.copy(); unsorted[row_ptr[3]:row_ptr[3] + 2] = unsorted[row_ptr[3]:row_ptr[3] + 2][::-1]
    bad = st.copy(); bad[5] = N
    s = np.zeros(NPAIRS); hit = np.zeros(NPAIRS, np.uint8)
    with Handle(N, 4, 4, A, None, 0, row_ptr, col) as ok:
        assert L.gemhip_eval_pairs(ok.h, NPAIRS, _hip.ptr(bad, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(s, C.c_double), None) == _hip.E_INVALID
        assert b'st[5] = 300 outside [0,300)' in L.gemhip_last_error()
        nodes = np.array([0, N], np.int32)
        assert L.gemhip_eval_ap(ok.h, 1, 2, _hip.ptr(nodes, C.c_int32), _hip.ptr(s, C.c_double)) == _hip.E_INVALID
    with Handle(N, 4, 4, A, None, 0, row_ptr, unsorted) as un:
        assert L.gemhip_eval_pairs(un.h, NPAIRS, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(s, C.c_double), _hip.ptr(hit, C.c_uint8)) == _hip.E_INVALID
        assert b'ascending' in L.gemhip_last_error()
        _hip.check(L.gemhip_eval_pairs(un.h, NPAIRS, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(s, C.c_double), None))   # scores alone do not need it


# ------------------------------------------------------------------ evaluate_reconstruction_gpu against the reference fixture
@pytest.mark.parametrize('name', sorted(CASES))
def test_gpu_evaluator_reproduces_the_reference(name, karate, sbm1024):
    c = CASES[name]
    G = karate if c['graph'] == 'karate' else sbm1024
    MAP, prec, err, base = gr.evaluate_reconstruction_gpu(G, model_of(c), embedding_of(c), edge_pairs=REF['pairs'][c['pairs']],
                                                          is_undirected=c['is_undirected'])
    print('%s: MAP %.17g (reference %.17g), curve entries differing: %d of %d' % (name, MAP, c['MAP'], int(np.sum(np.array(prec) != np.array(c['prec_curv'])))
                                                                                  if len(prec) == len(c['prec_curv']) else -1, len(c['prec_curv'])))
    if c['method'] == 'grid':
        assert MAP == c['MAP']                                     # half-integer coordinates: every score is exact
    assert abs(MAP - c['MAP']) <= 1e-12
    assert prec == c['prec_curv']
    assert err is None and base is None


def test_gpu_evaluator_on_an_edge_list_graph_and_with_a_drawn_sample(sbm1024):
    c = CASES['sbm1024_gf_undirected']
    n, src, dst, w, _ = edge_arrays(sbm1024)
    E = EdgeListGraph(n, src, dst, None)
    MAP, prec, _, _ = gr.evaluate_reconstruction_gpu(E, model_of(c), embedding_of(c), edge_pairs=np.array(REF['pairs'][c['pairs']]))
    assert abs(MAP - c['MAP']) <= 1e-12 and prec == c['prec_curv']
    X = embedding_of(c)
    got = gr.evaluate_reconstruction_gpu(E, model_of(c), X, sample_ratio_e=0.01, seed=5)
    want = gr.evaluateStaticGraphReconstruction(sbm1024, model_of(c), X, None, sample_ratio_e=0.01, seed=5)
    assert len(got[1]) == len(want[1]) and abs(got[0] - want[0]) <= 1e-12
    by_nodes = gr.evaluate_reconstruction_gpu(E, model_of(c), X, nodes=np.arange(0, n, 8))
    assert by_nodes[1] is None
    assert by_nodes[0] == pytest.approx(gr.sampled_ap_gpu(E, model_of(c), X, np.arange(0, n, 8)).mean(), abs=1e-15)
    with pytest.raises(ValueError):
        gr.evaluate_reconstruction_gpu(E, model_of(c), X)


@pytest.mark.parametrize('k', range(len(REF['weighted']['cases'])))
def test_gpu_weighted_edge_error(k):
    w = REF['weighted']['cases'][k]
    c = CASES['karate_%s_undirected' % w['method']]
    G = weighted_karate()
    for graph in (G, EdgeListGraph(*edge_arrays(G)[:4])):
        MAP, prec, err, base = gr.evaluate_reconstruction_gpu(graph, model_of(c), embedding_of(c), is_weighted=True)
        assert MAP is None and prec is None
        assert abs(err - w['err']) <= 1e-12 * w['err']
        assert abs(base - w['err_baseline']) <= 1e-12 * w['err_baseline']


def test_self_loop_contributes_its_squared_weight():
    G = EdgeListGraph(3, [0, 1, 1], [1, 1, 2], [2.0, 3.0, 0.0])                  # a self-loop of weight 3 and a zero-weight edge
    X = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 2.0]])
    _, _, err, base = gr.evaluate_reconstruction_gpu(G, None, X, is_weighted=True)
    assert err == pytest.approx(np.sqrt((2.0 - 0.5) ** 2 + 3.0 ** 2), rel=1e-15)
    assert base == pytest.approx(np.sqrt(13.0), rel=1e-15)


# ------------------------------------------------------------------ AP of Laplacian Eigenmaps / LLE (kind 1)
def distance_kernel_matrix(X, block=64):
    """exp(-norm(x_i - x_j)^2), the scalar get_edge_weight of lap.py:74 / lle.py:53, built by row blocks; zero diagonal."""
    n = X.shape[0]
    out = np.empty((n, n))
    for r in range(0, n, block):
        out[r:r + block] = np.exp(-np.linalg.norm(X[r:r + block, None, :] - X[None, :, :], axis=2) ** 2)
    np.fill_diagonal(out, 0.0)
    return out


def check_kind1(G, model, X, nodes=None):
    n = len(G.nodes)
    X32 = np.asarray(X).astype(np.float32).astype(np.float64)
    est = distance_kernel_matrix(X32)
    truth = gr._adjacency_bool(G, n)
    nodes = np.arange(n) if nodes is None else nodes
    for und in (True, False):
        ap = gr.sampled_ap_gpu(G, model, X32, nodes, is_undirected=und)
        ap_ref = gr.average_precision_rows(est, truth, undirected=und)[nodes]
        assert np.abs(ap - ap_ref).max() < 1e-9, (und, np.abs(ap - ap_ref).max())
    return est


def test_lap_and_lle_ap_on_the_karate_goldens(karate):
    check_kind1(karate, LaplacianEigenmaps(d=2), np.loadtxt(golden_path('ref_karate_LaplacianEigenmaps.txt')))
    check_kind1(karate, LocallyLinearEmbedding(d=2), np.loadtxt(golden_path('ref_karate_LocallyLinearEmbedding.txt')))


def test_lap_ap_on_sbm1024_with_an_underflowing_row(sbm1024):
    X = 0.5 * np.random.RandomState(2).randn(1024, 8)                          # squared distances of order 1: distinct distances, distinct exp
    X[5] += 14.0                                                               # node 5: ||x_5 - x_j||^2 ~ 8 * 196 > 800, exp underflows to 0
    est = check_kind1(sbm1024, LaplacianEigenmaps(d=8), X)
    assert np.all(est[5] == 0.0) and np.all(est[:, 5] == 0.0)                   # ... and falls out of the `> 0` filter on both sides
    check_kind1(sbm1024, LocallyLinearEmbedding(d=8), X[:, :3])


def test_kind1_ties_follow_the_stable_sort_rule(sbm1024):
    X = np.round(np.random.RandomState(0).randn(1024, 4) * 2) / 2               # coarse grid: exact squared distances, many exact ties
    check_kind1(sbm1024, LaplacianEigenmaps(d=4), X)


def test_kind1_hub_nodes_with_more_than_512_neighbours():
    n = 3000
    rng = np.random.RandomState(3)
    hub_nb = {0: rng.choice(np.arange(1, n), 1700, replace=False), 7: rng.choice(np.arange(8, n), 513, replace=False)}
    src = [rng.randint(0, n, 6000)]; dst = [rng.randint(0, n, 6000)]
    for h, nb in hub_nb.items():
        src.append(np.full(len(nb), h)); dst.append(nb)
    src = np.concatenate(src); dst = np.concatenate(dst)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    key = np.unique(np.minimum(src, dst) * n + np.maximum(src, dst))
    a, b = key // n, key % n
    G = EdgeListGraph(n, np.concatenate([a, b]), np.concatenate([b, a]), None)
    check_kind1(G, LaplacianEigenmaps(d=16), rng.randn(n, 16) * 0.3, nodes=np.array([0, 7, 1, 2999, 1500], dtype=np.int32))


# ------------------------------------------------------------------ the one-shot entry point
def test_one_shot_entry_point_equals_the_handle(sbm1024):
    n, src, dst, w, _ = edge_arrays(sbm1024)
    row_ptr, col, _ = to_csr(n, src, dst, None)                                  # unsorted columns: the AP path does not need them sorted
    X = np.load(golden_path('hope_sbm1024_d32.npz'))['X']
    A = np.ascontiguousarray(X[:, :16], dtype=np.float32); B = np.ascontiguousarray(X[:, 16:], dtype=np.float32)
    nodes = np.arange(0, n, 3, dtype=np.int32)
    for und in (1, 0):
        for Bm in (B, None):
            old = np.zeros(len(nodes))
            _hip.check(_hip.lib().gemhip_eval_sampled_ap(n, 16, 16, _hip.ptr(A, C.c_float), _hip.ptr(Bm, C.c_float), _hip.ptr(row_ptr, C.c_int64),
                                                         _hip.ptr(col, C.c_int32), und, len(nodes), _hip.ptr(nodes, C.c_int32), _hip.ptr(old, C.c_double)))
            with Handle(n, 16, 16, A, Bm, 0, row_ptr, col) as h:
                new = h.ap(nodes, und)
            assert old.tobytes() == new.tobytes() and old.max() > 0
