"""GPU: gem_amd/csrc/cc.hip -- gemhip_cc_labels (cc_init / cc_union / cc_flatten / cc_sizes / cc_winner kernels) and gemhip_lcc (the same plus the
two three-kernel compactions) -- against the host restatement of get_lcc in tests/lcc_refs.py.  Everything is integers or copied bits: every
comparison is exact (array_equal; weights as their 32-bit patterns).  Output buffers are pre-filled with a sentinel, so the tests also pin that
nothing past n_out / m_out is written.

Sizes of the scans (cc.hip): 4 elements per thread, 256 per wavefront, 1024 per workgroup (SCAN_TILE), 1024 tile counts per pass of the one
workgroup that scans them (SUMS_BLOCK) -- so 1024 * 1024 elements is the first size at which that kernel needs a second pass with a carry."""
import ctypes as C
import functools

import numpy as np
import pytest

import lcc_refs
from gem_amd import _hip
from gem_amd.graph import EdgeListGraph, connected_components, largest_component, rmat_graph

pytestmark = pytest.mark.gpu

SENTINEL = -9


def run_labels(n, src, dst):
    src = _hip.as_i32(src); dst = _hip.as_i32(dst)
    labels = np.full(n, SENTINEL, np.int32); nc = C.c_int32(SENTINEL)
    _hip.check(_hip.lib().gemhip_cc_labels(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(labels, C.c_int32), C.byref(nc)))
    return nc.value, labels


def run_lcc(n, src, dst, w=None):
    """Every output of gemhip_lcc, whole buffers (the part the call must leave alone still holds the sentinel)."""
    src = _hip.as_i32(src); dst = _hip.as_i32(dst); w = _hip.as_f32(w)
    m = len(src)
    out = {k: np.full(size, SENTINEL, np.int32) for k, size in (('old_of_new', n), ('new_of_old', n), ('src', m), ('dst', m))}
    w_out = None if w is None else np.full(m, SENTINEL, np.int32).view(np.float32)
    n_out, m_out, nc = C.c_int64(SENTINEL), C.c_int64(SENTINEL), C.c_int32(SENTINEL)
    _hip.check(_hip.lib().gemhip_lcc(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(w, C.c_float), C.byref(n_out), C.byref(m_out),
                                     _hip.ptr(out['old_of_new'], C.c_int32), _hip.ptr(out['new_of_old'], C.c_int32), _hip.ptr(out['src'], C.c_int32),
                                     _hip.ptr(out['dst'], C.c_int32), _hip.ptr(w_out, C.c_float), C.byref(nc)))
    out.update(n_out=n_out.value, m_out=m_out.value, n_components=nc.value, w=None if w_out is None else w_out.view(np.int32))
    return out


def check_against_restatement(n, src, dst, w=None):
    """gemhip_cc_labels and gemhip_lcc of one graph equal lcc_refs, output by output.  Returns (restatement, device outputs)."""
    ref = lcc_refs.lcc(n, src, dst, w)
    nc, labels = run_labels(n, src, dst)
    assert nc == ref['n_components'] and np.array_equal(labels, ref['labels'])
    got = run_lcc(n, src, dst, w)
    k, mk = len(ref['old_of_new']), len(ref['src'])
    assert (got['n_out'], got['m_out'], got['n_components']) == (k, mk, ref['n_components'])
    assert np.array_equal(got['new_of_old'], ref['new_of_old'])
    assert np.array_equal(got['old_of_new'][:k], ref['old_of_new']) and np.all(got['old_of_new'][k:] == SENTINEL)
    assert np.array_equal(got['src'][:mk], ref['src']) and np.all(got['src'][mk:] == SENTINEL)
    assert np.array_equal(got['dst'][:mk], ref['dst']) and np.all(got['dst'][mk:] == SENTINEL)
    if w is not None:
        assert np.array_equal(got['w'][:mk], ref['w'].view(np.int32)) and np.all(got['w'][mk:] == SENTINEL)
    return ref, got


def random_bits_f32(rng, m):
    """Weights as arbitrary 32-bit patterns (NaNs, infinities, denormals, -0.0 among them): carried bit for bit or not at all."""
    return rng.randint(-2 ** 31, 2 ** 31, size=m, dtype=np.int64).astype(np.int32).view(np.float32)


# ------------------------------------------------------------------ 1. a hand-written graph
def test_hand_written_graph():
    """12 nodes.  {2,5,7,9,11}: {9,11} and {2,5,7} hang together by the one-way arc 9 -> 5 alone, 11 -> 9 is listed twice.  {0,3,4}: holds the smallest
    id but is the smaller one; 3 -> 0 twice, a self-loop on 0.  1, 6, 8 isolated; 10 isolated with a self-loop.  Arcs in descending order of source."""
    src = np.array([11, 11, 10, 9, 7, 7, 5, 4, 3, 3, 0], np.int32)
    dst = np.array([9, 9, 10, 5, 5, 2, 2, 3, 0, 0, 0], np.int32)
    w = (np.arange(11) * 0.5 + 0.25).astype(np.float32)
    nc, labels = run_labels(12, src, dst)
    assert nc == 6 and labels.tolist() == [0, 1, 2, 0, 0, 2, 6, 2, 8, 2, 10, 2]
    got = run_lcc(12, src, dst, w)
    assert (got['n_out'], got['m_out'], got['n_components']) == (5, 6, 6)
    assert got['old_of_new'].tolist() == [2, 5, 7, 9, 11] + [SENTINEL] * 7
    assert got['new_of_old'].tolist() == [-1, -1, 0, -1, -1, 1, -1, 2, -1, 3, -1, 4]
    assert got['src'][:6].tolist() == [4, 4, 3, 2, 2, 1] and got['dst'][:6].tolist() == [3, 3, 1, 1, 0, 0]
    assert got['w'][:6].view(np.float32).tolist() == [0.25, 0.75, 1.75, 2.25, 2.75, 3.25]
    check_against_restatement(12, src, dst, w)
    # the Python layer on the same graph
    assert connected_components(EdgeListGraph(12, src, dst, w))[0] == 6
    g, old = largest_component(EdgeListGraph(12, src, dst, w))
    assert (g.n, g.src.tolist(), g.dst.tolist(), old.tolist()) == (5, [4, 4, 3, 2, 2, 1], [3, 3, 1, 1, 0, 0], [2, 5, 7, 9, 11])
    g, old = largest_component(EdgeListGraph(12, src, dst))                    # unweighted: no weights come back
    assert g.w is None and g.src.tolist() == [4, 4, 3, 2, 2, 1]


# ------------------------------------------------------------------ 2. deep trees
@pytest.mark.parametrize('variant', ['ascending', 'descending', 'permuted'])
def test_path_of_5000_nodes(variant):
    n = 5000
    rng = np.random.RandomState(11)
    ids = {'ascending': np.arange(n), 'descending': np.arange(n)[::-1], 'permuted': rng.permutation(n)}[variant]
    src, dst = ids[:-1].copy(), ids[1:].copy()
    if variant == 'permuted':
        order = rng.permutation(n - 1)
        src, dst = src[order], dst[order]
    nc, labels = run_labels(n, src, dst)
    assert nc == 1 and not labels.any()
    ref, got = check_against_restatement(n, src, dst, random_bits_f32(rng, n - 1))
    assert got['n_out'] == n and got['m_out'] == n - 1


# ------------------------------------------------------------------ 3. one root takes every CAS and every histogram add
@pytest.mark.parametrize('hub_last', [False, True])
def test_star_of_70000_leaves(hub_last):
    n = 70001
    rng = np.random.RandomState(12)
    hub = n - 1 if hub_last else 0
    leaves = np.delete(np.arange(n), hub)
    out = rng.rand(n - 1) < 0.5                                                # half the arcs point at the hub, half away from it
    src = np.where(out, hub, leaves); dst = np.where(out, leaves, hub)
    nc, labels = run_labels(n, src, dst)
    assert nc == 1 and not labels.any()
    check_against_restatement(n, src, dst)


# ------------------------------------------------------------------ 4. debris
def test_debris_around_a_triangle():
    """3000 isolated edges, 500 isolated nodes, one triangle, ids shuffled: 3501 components, thousands of candidates for the arg-max, nearly
    every lane of a wavefront with a label of its own in the histogram."""
    rng = np.random.RandomState(13)
    n = 6000 + 500 + 3
    ids = rng.permutation(n)
    a, b = ids[0:6000:2], ids[1:6000:2]
    t = ids[6500:]
    src = np.concatenate([a, [t[0], t[1], t[2]]]); dst = np.concatenate([b, [t[1], t[2], t[0]]])
    order = rng.permutation(len(src))
    src, dst = src[order], dst[order]
    ref, got = check_against_restatement(n, src, dst, random_bits_f32(rng, len(src)))
    assert got['n_components'] == 3501 and got['n_out'] == 3 and got['m_out'] == 3
    assert sorted(got['old_of_new'][:3].tolist()) == sorted(t.tolist())


# ------------------------------------------------------------------ 5. ties
def test_tie_goes_to_the_component_with_the_smallest_id():
    """Two components of 100 nodes, the evens and the odds below 200, and one of 50 nodes: the evens hold node 0 and win."""
    rng = np.random.RandomState(14)
    ev = rng.permutation(np.arange(0, 200, 2)); od = rng.permutation(np.arange(1, 200, 2)); sm = rng.permutation(np.arange(200, 250))
    src = np.concatenate([od[:-1], sm[:-1], ev[:-1]]); dst = np.concatenate([od[1:], sm[1:], ev[1:]])
    ref, got = check_against_restatement(250, src, dst)
    assert got['n_components'] == 3 and got['old_of_new'][:got['n_out']].tolist() == list(range(0, 200, 2))


def test_the_larger_component_wins_over_the_one_with_the_smallest_id():
    rng = np.random.RandomState(15)
    small = np.arange(0, 60); big = np.arange(60, 200)
    src = np.concatenate([small[:-1], big[:-1]]); dst = np.concatenate([small[1:], big[1:]])
    order = rng.permutation(len(src))
    ref, got = check_against_restatement(200, src[order], dst[order])
    assert got['n_components'] == 2 and got['old_of_new'][:got['n_out']].tolist() == big.tolist()


# ------------------------------------------------------------------ 6. the edges of the scans
@functools.lru_cache(maxsize=None)
def alternating_graph(n, kept_arcs, dropped_arcs, seed):
    """Even ids form one component (a random tree over them plus random extra arcs: kept_arcs arcs in all), odd ids are debris (self-loops and
    arcs inside the pairs {4j+1, 4j+3}: dropped_arcs arcs) -- kept and dropped NODES alternate, kept and dropped ARCS are shuffled together."""
    rng = np.random.RandomState(seed)
    even = np.arange(0, n, 2); odd = np.arange(1, n, 2)
    k = len(even)
    assert kept_arcs >= k - 1 and k >= 2 and len(odd) >= 1
    child = np.arange(1, k)
    parent = (rng.rand(k - 1) * child).astype(np.int64)                        # a random recursive tree: node c hangs under one of 0..c-1
    extra = kept_arcs - (k - 1)
    a = np.concatenate([even[child], even[rng.randint(0, k, extra)]]); b = np.concatenate([even[parent], even[rng.randint(0, k, extra)]])
    o = rng.randint(0, len(odd), dropped_arcs)
    partner = np.minimum(o ^ 1, len(odd) - 1)                                  # the other odd id of the pair (or itself at the ragged end)
    loop = rng.rand(dropped_arcs) < 0.3
    a = np.concatenate([a, odd[o]]); b = np.concatenate([b, np.where(loop, odd[o], odd[partner])])
    flip = rng.rand(len(a)) < 0.5
    src = np.where(flip, b, a); dst = np.where(flip, a, b)
    order = rng.permutation(len(src))
    src = src[order].astype(np.int32); dst = dst[order].astype(np.int32)
    return src, dst, random_bits_f32(rng, len(src))


SCAN_SIZES = sorted(s + d for s in (4, 256, 1024, 2048, 1024 * 1024) for d in (-1, 0, 1))


@pytest.mark.parametrize('size', SCAN_SIZES)
def test_scan_edges(size):
    """n = size nodes, size kept arcs among 2 * size + 1 arcs (so the arc scan has a ragged last tile and, at the large sizes, several passes of the
    tile-count scan as well); 1024 * 1024 + 1 nodes need every level of the node scan: 1025 tile counts, a second pass with a carry."""
    src, dst, w = alternating_graph(size, size, size + 1, seed=size)
    ref, got = check_against_restatement(size, src, dst, w)
    assert got['n_out'] == (size + 1) // 2 and got['m_out'] == size
    assert np.array_equal(got['old_of_new'][:got['n_out']], np.arange(0, size, 2))


# ------------------------------------------------------------------ 7. the smallest inputs
def test_no_arcs_and_one_node():
    none = np.zeros(0, np.int32)
    nc, labels = run_labels(5, none, none)
    assert nc == 5 and labels.tolist() == [0, 1, 2, 3, 4]
    got = run_lcc(5, none, none)
    assert (got['n_out'], got['m_out'], got['n_components']) == (1, 0, 5)                  # every node its own component: node 0 wins
    assert got['old_of_new'].tolist() == [0] + [SENTINEL] * 4 and got['new_of_old'].tolist() == [0, -1, -1, -1, -1]
    L = _hip.lib()                                                                         # m = 0 with NULL arc pointers, in and out
    n_out, m_out, ncc = C.c_int64(), C.c_int64(), C.c_int32()
    o = np.zeros(5, np.int32); nn = np.zeros(5, np.int32)
    _hip.check(L.gemhip_lcc(5, 0, None, None, None, C.byref(n_out), C.byref(m_out), _hip.ptr(o, C.c_int32), _hip.ptr(nn, C.c_int32), None, None, None,
                            C.byref(ncc)))
    assert (n_out.value, m_out.value, ncc.value) == (1, 0, 5)
    nc, labels = run_labels(1, none, none)
    assert nc == 1 and labels.tolist() == [0]
    got = run_lcc(1, none, none)
    assert (got['n_out'], got['m_out'], got['n_components'], got['old_of_new'].tolist(), got['new_of_old'].tolist()) == (1, 0, 1, [0], [0])
    got = run_lcc(1, [0, 0], [0, 0], np.array([1.5, -2.5], np.float32))                    # one node, its self-loop twice
    assert (got['n_out'], got['m_out'], got['src'].tolist(), got['dst'].tolist()) == (1, 2, [0, 0], [0, 0])
    assert got['w'].view(np.float32).tolist() == [1.5, -2.5]


# ------------------------------------------------------------------ 8. the benchmark's power-law graph; 10. twice the same
def test_rmat_scale_14_and_reproducibility():
    g = rmat_graph(14, 65536, 5)
    rng = np.random.RandomState(16)
    w = random_bits_f32(rng, len(g.src))
    ref, got = check_against_restatement(g.n, g.src, g.dst, w)
    assert got['n_components'] == 8942 and got['n_out'] == 7403
    again = run_lcc(g.n, g.src, g.dst, w)
    for key in ('n_out', 'm_out', 'n_components'):
        assert again[key] == got[key]
    for key in ('old_of_new', 'new_of_old', 'src', 'dst', 'w'):
        assert np.array_equal(again[key], got[key]), key
    assert np.array_equal(run_labels(g.n, g.src, g.dst)[1], run_labels(g.n, g.src, g.dst)[1])
    ph = _hip.last_call_phases()                                                           # gemhip_last_call_phases covers these calls
    assert ph['library_call_s'] > 0 and ph['kernels_s'] > 0 and ph['h2d_s'] > 0 and ph['d2h_s'] > 0
    assert ph['library_call_s'] >= ph['kernels_s']


# ------------------------------------------------------------------ 9. plug-in level
def test_get_lcc_on_a_karate_train_split(karate):
    from gem.utils import graph_util
    from gem_amd.graph import edge_arrays
    train, _ = lcc_refs.karate_train_split(karate, 0.5)
    nx_train = train.to_networkx()
    n, src, dst, w, _ = edge_arrays(nx_train)                                              # the arcs as networkx iterates them
    ref = lcc_refs.lcc(n, src, dst, w)
    G, node_map = graph_util.get_lcc(nx_train)
    assert node_map == dict(zip(ref['old_of_new'].tolist(), range(27)))
    assert list(G.nodes()) == list(range(27)) and G.is_directed()
    assert sorted(G.edges(data='weight')) == sorted(zip(ref['src'].tolist(), ref['dst'].tolist(), ref['w'].astype(np.float64).tolist()))
    ref = lcc_refs.lcc(train.n, train.src, train.dst, train.w)
    g, new_of_old = graph_util.get_lcc(train)                                              # the array form
    assert isinstance(g, EdgeListGraph) and g.n == 27 and np.array_equal(new_of_old, ref['new_of_old'])
    assert np.array_equal(g.src, ref['src']) and np.array_equal(g.dst, ref['dst']) and np.array_equal(g.w, ref['w'])


def test_link_prediction_on_the_largest_component_of_the_train_graph(karate):
    from gem_amd.embedding.gf import GraphFactorization
    from gem_amd.evaluation import link_prediction as lp
    from gem_amd.evaluation import reconstruction as gr
    model = GraphFactorization(d=4, eta=0.05, regu=0.1, max_iter=200)
    np.random.seed(7)
    MAP, prec = lp.evaluateStaticLinkPrediction(karate, model, train_ratio=0.5, lcc=True)
    X = model.get_embedding()
    assert X.shape == (27, 4)
    train, test = lcc_refs.karate_train_split(karate, 0.5)                                 # the same split: the same seed
    ref = lcc_refs.lcc(train.n, train.src, train.dst, train.w)
    ts, td = lcc_refs.restrict_test(ref['new_of_old'], test.src, test.dst)
    train_truth = np.zeros((27, 27), bool); train_truth[ref['src'], ref['dst']] = True
    test_truth = np.zeros((27, 27), bool); test_truth[ts, td] = True
    want_MAP, want_prec = lp.link_prediction_dense(model.get_reconstructed_adj(X), train_truth, test_truth, True)
    assert MAP == want_MAP and prec == want_prec
    assert test_truth.any() and MAP > 0
    # `nodes` are old ids: mapped, the dropped ones left out (node 0 is kept; the dropped ones are whatever the split isolated)
    dropped = np.flatnonzero(ref['new_of_old'] < 0)
    kept = ref['old_of_new'][:5]
    np.random.seed(7)
    some, _ = lp.evaluateStaticLinkPrediction(karate, model, train_ratio=0.5, nodes=np.concatenate([dropped, kept]), lcc=True)
    np.random.seed(7)
    same, _ = lp.evaluateStaticLinkPrediction(karate, model, train_ratio=0.5, nodes=kept, lcc=True)
    assert some == same
