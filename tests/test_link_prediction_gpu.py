"""GPU: link prediction on the evaluator handle of gem_amd/csrc/eval.hip -- gemhip_eval_set_mask, gemhip_eval_ap_masked (eval_ap_kernel<NV, KIND, MASKED>)
and gemhip_eval_topk (eval_topk_kernel) -- node by node over all 700 nodes of instrument_refs.ap_graph with the train mask of linkpred_refs
(an empty mask row on the hub, a mask row longer than a chunk, a node whose candidates are exactly its positives, a node with every positive
masked, an unsorted row with a duplicate, a masked self-loop, a row of lower ids only), against link_prediction_rows and the stable host order
on the dense fp64 scores of the same fp32 inputs.  Bars: instrument_refs.AP_GRID_BAR on the half-integer grid family (exact scores, ties
everywhere: the id order itself is the test), AP_RANDOM_BAR on the random family after checking on the CPU that the fp64 reference is clear of
ties (every (da, kind) used here is one of instrument_refs.AP_CASES, whose seeds test_instrument_refs.py checks too)."""
import ctypes as C
import functools

import numpy as np
import pytest

import instrument_refs as ir
import linkpred_refs as lr
from gem_amd import _hip
from gem_amd.evaluation import link_prediction as lp
from gem_amd.evaluation import reconstruction as gr
from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
from test_eval_pairs_gpu import Handle

pytestmark = pytest.mark.gpu

N = ir.AP_N
# (da, pad, kind, split): the issue's widths (257 with ld = da + 3), one HOPE split, one distance-kernel width
AP_CASES = [(1, 0, 0, False), (64, 0, 0, False), (65, 0, 0, False), (128, 0, 0, False), (257, 3, 0, False), (512, 0, 0, False), (91, 0, 0, True),
            (65, 0, 1, False)]
# every eval_topk_kernel<NV, KIND> instantiation: NV = 1, 2, 4, 8 for both kinds, and a HOPE split
TOPK_CASES = [(64, 0, 0, False), (65, 0, 0, False), (182, 0, 0, False), (257, 3, 0, False), (91, 0, 0, True),
              (63, 0, 1, False), (65, 0, 1, False), (182, 0, 1, False), (257, 0, 1, False)]
ALL_NODES = np.arange(N, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def graph():
    """(row_ptr, col, truth) of the test graph as ap_graph gives it (row 20 unsorted), its column-sorted CSR for top-k, and the train mask."""
    row_ptr, col, truth = ir.ap_graph()
    rs, cs = np.nonzero(truth)
    srp = np.zeros(N + 1, np.int64); np.cumsum(np.bincount(rs, minlength=N), out=srp[1:])
    mrp, mcol, train = lr.lp_mask(truth)
    return row_ptr, col, truth, srp, cs.astype(np.int32), mrp, mcol, train


@functools.lru_cache(maxsize=None)
def problem(da, pad, kind, split, family):
    """Operands and the dense fp64 reference of one case, computed once and shared (read-only) by every test that needs them."""
    A, B = ir.ap_operands(da, pad, kind, split, family, seed=ir.ap_seed(da, kind))
    score, mag = ir.ap_dense_scores(A, B, da, kind)
    if family == 'random':
        assert ir.ap_reference_is_clear_of_ties(score, mag, da), 'the fp64 reference does not decide an order at this seed: pick another'
    score.setflags(write=False)
    return A, B, score


def set_mask(h, mrp, mcol):
    return _hip.lib().gemhip_eval_set_mask(h.h, _hip.ptr(mrp, C.c_int64), _hip.ptr(mcol, C.c_int32))


def ap_masked(h, nodes, undirected):
    out = np.full(len(nodes), np.nan); npos = np.full(len(nodes), -7, np.int64)
    _hip.check(_hip.lib().gemhip_eval_ap_masked(h.h, int(undirected), len(nodes), _hip.ptr(nodes, C.c_int32), _hip.ptr(out, C.c_double), _hip.ptr(npos, C.c_int64)))
    return out, npos


def topk(h, nodes, k, undirected, use_mask):
    ids = np.full((len(nodes), k), -9, np.int32); score = np.full((len(nodes), k), np.nan); hit = np.full((len(nodes), k), 7, np.uint8)
    _hip.check(_hip.lib().gemhip_eval_topk(h.h, int(undirected), int(use_mask), len(nodes), _hip.ptr(nodes, C.c_int32), k, _hip.ptr(ids, C.c_int32),
                                           _hip.ptr(score, C.c_double), _hip.ptr(hit, C.c_uint8)))
    return ids, score, hit


# ------------------------------------------------------------------ 1. masked AP of all 700 nodes
@pytest.mark.parametrize('family', ['grid', 'random'])
@pytest.mark.parametrize('da,pad,kind,split', AP_CASES)
def test_masked_ap_of_every_node(da, pad, kind, split, family):
    row_ptr, col, truth, _, _, mrp, mcol, train = graph()
    bar = ir.AP_GRID_BAR if family == 'grid' else ir.AP_RANDOM_BAR
    A, B, score = problem(da, pad, kind, split, family)
    with Handle(N, da, da + pad, A, B, kind, row_ptr, col) as h:
        _hip.check(set_mask(h, mrp, mcol))
        got = {und: ap_masked(h, ALL_NODES, und) for und in (True, False)}
        plain = h.ap(ALL_NODES, False)                                # gemhip_eval_ap ignores the handle's mask
    for und in (True, False):
        ap, npos = got[und]
        ref = lp.link_prediction_rows(score, train, truth, undirected=und)
        err = np.abs(ap - ref)
        print('masked AP %s kind %d da=%d ld=%d split=%d undirected=%d: max |AP - ref| = %.3g at node %d (bar %.0e), MAP %.6f'
              % (family, kind, da, da + pad, split, und, err.max(), int(err.argmax()), bar, ap.mean()))
        assert np.all(err <= bar)
        assert np.array_equal(npos, lr.npos_reference(score, train, truth, und))
        assert ap[lr.LP_ALL_MASKED] == 0.0 and npos[lr.LP_ALL_MASKED] == 0 and ap[ir.AP_EMPTY] == 0.0 and npos[ir.AP_EMPTY] == 0
        if da > 1:
            assert ap[ir.AP_513] == 1.0 and npos[ir.AP_513] > 0        # every stranger masked: the positives take the first ranks
            assert 0 < npos[ir.AP_512] <= 112 and npos[ir.AP_HUB] > 0    # 400 of node 5's 512 test neighbours are train arcs
    assert np.all(np.abs(plain - gr.average_precision_rows(score, truth, undirected=False)) <= bar)
    assert not np.array_equal(plain, got[False][0])


# ------------------------------------------------------------------ 2. no mask, empty mask, cleared mask: the bytes of gemhip_eval_ap
@pytest.mark.parametrize('da,pad,kind,split', [(65, 0, 0, False), (257, 3, 0, False), (91, 0, 0, True), (65, 0, 1, False)])
def test_without_a_mask_the_bytes_are_those_of_eval_ap(da, pad, kind, split):
    row_ptr, col, truth, _, _, mrp, mcol, train = graph()
    A, B, score = problem(da, pad, kind, split, 'grid')
    empty_rp = np.zeros(N + 1, np.int64)
    with Handle(N, da, da + pad, A, B, kind, row_ptr, col) as h:
        for und in (True, False):
            want = h.ap(ALL_NODES, und)
            none, npos = ap_masked(h, ALL_NODES, und)
            assert none.tobytes() == want.tobytes()
            assert np.array_equal(npos, lr.npos_reference(score, np.zeros_like(train), truth, und))
            _hip.check(set_mask(h, empty_rp, None))
            assert ap_masked(h, ALL_NODES, und)[0].tobytes() == want.tobytes()
            _hip.check(set_mask(h, mrp, mcol))
            assert ap_masked(h, ALL_NODES, und)[0].tobytes() != want.tobytes()
            _hip.check(set_mask(h, None, None))
            assert ap_masked(h, ALL_NODES, und)[0].tobytes() == want.tobytes()


# ------------------------------------------------------------------ 3. top-k
def check_topk(h, score, truth, train, k, masked, bar):
    for und in (True, False):
        ids, s, hit = topk(h, ALL_NODES, k, und, masked)
        again = topk(h, ALL_NODES, k, und, masked)
        assert all(x.tobytes() == y.tobytes() for x, y in zip((ids, s, hit), again))           # deterministic: the same bytes on every call
        short = 0
        for i in range(N):
            order = lr.candidate_order(score[i], i, und, train[i] if masked else None)
            m = min(k, len(order))
            short += m < k
            assert np.array_equal(ids[i, :m], order[:m]), (i, und)
            assert np.all(ids[i, m:] == -1) and np.all(s[i, m:] == 0.0) and np.all(hit[i, m:] == 0)
            assert np.all(np.abs(s[i, :m] - score[i, order[:m]]) <= bar)
            assert np.array_equal(hit[i, :m].astype(bool), truth[i, order[:m]])
            # precision@1..m from the top-k hits = the head of node i's precision curve from the dense matrix
            assert np.array_equal(np.cumsum(hit[i, :m]) / np.arange(1, m + 1), np.cumsum(truth[i, order])[:m] / np.arange(1, m + 1))
        assert short == N if k >= N else (short > 0 or not und)                                  # padding is exercised: k = 1000 pads every node, node 699 has no j > i
    return ids


@pytest.mark.parametrize('family', ['grid', 'random'])
@pytest.mark.parametrize('masked', [True, False])
@pytest.mark.parametrize('k', [1, 10, 64, 100, 1000])
def test_topk_is_the_stable_host_order(k, masked, family):
    _, _, truth, srp, scol, mrp, mcol, train = graph()
    A, B, score = problem(65, 0, 0, False, family)
    with Handle(N, 65, 65, A, B, 0, srp, scol) as h:
        _hip.check(set_mask(h, mrp, mcol))                            # set in both runs: use_mask = 0 must ignore it
        check_topk(h, score, truth, train, k, masked, ir.AP_GRID_BAR if family == 'grid' else ir.AP_RANDOM_BAR)


@pytest.mark.parametrize('family', ['grid', 'random'])
@pytest.mark.parametrize('da,pad,kind,split', TOPK_CASES)
def test_topk_at_every_instantiation(da, pad, kind, split, family):
    _, _, truth, srp, scol, mrp, mcol, train = graph()
    A, B, score = problem(da, pad, kind, split, family)
    with Handle(N, da, da + pad, A, B, kind, srp, scol) as h:
        _hip.check(set_mask(h, mrp, mcol))
        ids = check_topk(h, score, truth, train, 100, True, ir.AP_GRID_BAR if family == 'grid' else ir.AP_RANDOM_BAR)
        assert set(ids[ir.AP_513][ids[ir.AP_513] >= 0]) <= set(np.flatnonzero(truth[ir.AP_513]))      # only its positives are left to rank
        # use_mask = 1 without a mask is the unmasked ranking
        _hip.check(set_mask(h, None, None))
        assert topk(h, ALL_NODES[:50], 7, True, 1)[0].tobytes() == topk(h, ALL_NODES[:50], 7, True, 0)[0].tobytes()


# ------------------------------------------------------------------ 4. refusals without a launch
def test_refusals():
    row_ptr, col, truth, srp, scol, mrp, mcol, train = graph()
    A, B, score = problem(65, 0, 0, False, 'grid')
    L = _hip.lib()
    ids = np.zeros((2, 1025), np.int32); s = np.zeros((2, 1025)); hit = np.zeros((2, 1025), np.uint8); ap = np.zeros(2)
    two = np.array([3, 4], np.int32); bad_node = np.array([3, N], np.int32)

    def refused(rc, words):
        assert rc == _hip.E_INVALID
        assert words in L.gemhip_last_error(), L.gemhip_last_error()

    def call_topk(h, nodes, k):
        return L.gemhip_eval_topk(h.h, 1, 1, 2, _hip.ptr(nodes, C.c_int32), k, _hip.ptr(ids, C.c_int32), _hip.ptr(s, C.c_double), _hip.ptr(hit, C.c_uint8))
    with Handle(N, 65, 65, A, B, 0, srp, scol) as h:
        _hip.check(set_mask(h, mrp, mcol))
        want = ap_masked(h, ALL_NODES, True)[0]
        bad_col = mcol.copy(); bad_col[17] = N
        refused(set_mask(h, mrp, bad_col), b'eval_set_mask: column 700 outside [0,700)')
        bad_rp = mrp.copy(); bad_rp[100] = bad_rp[99] - 1
        refused(set_mask(h, bad_rp, mcol), b'eval_set_mask: row_ptr decreases at row 99')
        bad_rp = mrp.copy(); bad_rp[0] = 1
        refused(set_mask(h, bad_rp, mcol), b'eval_set_mask: row_ptr[0] is 1, not 0')
        assert ap_masked(h, ALL_NODES, True)[0].tobytes() == want.tobytes()                   # a refused mask leaves the handle's mask as it was
        refused(call_topk(h, two, 0), b'eval_topk: k = 0 outside [1,1024]')
        refused(call_topk(h, two, 1025), b'eval_topk: k = 1025 outside [1,1024]')
        refused(call_topk(h, bad_node, 5), b'eval_topk: node 700 outside [0,700)')
        refused(L.gemhip_eval_ap_masked(h.h, 1, 2, _hip.ptr(bad_node, C.c_int32), _hip.ptr(ap, C.c_double), None), b'eval_ap_masked: node 700 outside [0,700)')
        _hip.check(L.gemhip_eval_topk(h.h, 1, 1, 0, None, 5, None, None, None))                # nsample = 0 is legal
        _hip.check(L.gemhip_eval_ap_masked(h.h, 1, 2, _hip.ptr(two, C.c_int32), _hip.ptr(ap, C.c_double), None))      # npos_out may be NULL
    assert not np.any(ids) and not np.any(s) and not np.any(hit)                             # nothing was written by a refused call
    with Handle(N, 65, 65, A, B, 0, row_ptr, col) as un:                                     # row 20 of ap_graph's own CSR is unsorted
        refused(call_topk(un, two, 5), b'eval_topk: the edge lookup needs every CSR row')
        _hip.check(L.gemhip_eval_ap_masked(un.h, 1, 2, _hip.ptr(two, C.c_int32), _hip.ptr(ap, C.c_double), None))     # AP does not need sorted rows


# ------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize('gname', ['karate', 'sbm1024'])
def test_end_to_end_against_the_dense_host_path(gname, karate, sbm1024):
    from gem_amd.embedding.gf import GraphFactorization
    G, und = (karate, False) if gname == 'karate' else (sbm1024, True)
    n = len(G.nodes)
    np.random.seed(23)
    train, test = split_di_graph_to_train_test(G, 0.8, is_undirected=und)
    model = GraphFactorization(d=4, max_iter=200, eta=0.01, regu=0.1, seed=3) if gname == 'karate' else \
        GraphFactorization(d=32, max_iter=50, eta=0.02, regu=0.01, seed=3)
    X = model.learn_embedding(graph=train)
    score = model.get_reconstructed_adj(X)
    train_t = gr._adjacency_bool(train, n); test_t = gr._adjacency_bool(test, n)
    k = 10
    res = lp.evaluate_link_prediction_gpu(train, test, model, X, nodes=np.arange(n), k=k, is_undirected=und)
    ref = lp.link_prediction_rows(score, train_t, test_t, undirected=und)
    err = np.abs(res['ap'] - ref)
    print('%s: link-prediction MAP %.6f (dense %.6f), max |AP - dense| = %.3g' % (gname, res['MAP'], lp.link_prediction_dense(score, train_t, test_t, und)[0], err.max()))
    assert np.all(err <= 1e-9)
    assert abs(res['MAP'] - lp.link_prediction_dense(score, train_t, test_t, und)[0]) <= 1e-9
    assert res['MAP'] > 0.0
    assert np.array_equal(res['npos'], lr.npos_reference(score, train_t, test_t, und))
    hits = np.array([test_t[i, lr.candidate_order(score[i], i, und, train_t[i])[:k]].sum() for i in range(n)])
    assert np.array_equal(res['hits_at_k'], hits) and np.array_equal(res['precision_at_k'], hits / float(k))
    listed = res['topk_id'] >= 0
    assert res['topk_id'].shape == (n, k) and not train_t[np.repeat(np.arange(n), k).reshape(n, k)[listed], res['topk_id'][listed]].any()      # no train arc is recommended
    # the pairs path = the dense evaluator restricted to the same pairs
    pairs = gr.random_edge_pairs(n, 0.05 if gname == 'sbm1024' else 0.5, und, seed=4)
    MAP, prec = lp.evaluate_link_prediction_gpu(train, test, model, X, edge_pairs=pairs, is_undirected=und)
    st, ed = pairs[:, 0], pairs[:, 1]
    keep = ~train_t[st, ed]
    assert 0 < keep.sum() < len(st)
    MAP_ref, prec_ref = gr.pair_metrics(n, st[keep], ed[keep], score[st[keep], ed[keep]], test_t[st[keep], ed[keep]], und, out_degree=test_t.sum(axis=1))
    assert abs(MAP - MAP_ref) <= 1e-9 and len(prec) == len(prec_ref) and np.all(np.abs(np.array(prec) - np.array(prec_ref)) <= 1e-9)
    same = lp.evaluate_link_prediction_gpu(train, test, model, X, sample_ratio_e=0.05 if gname == 'sbm1024' else 0.5, is_undirected=und, seed=4)
    assert same[0] == MAP and same[1] == prec
