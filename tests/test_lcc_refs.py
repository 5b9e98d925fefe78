"""CPU: tests/lcc_refs.py -- the restatement of get_lcc (gem/utils/graph_util.py:29-34) the GPU tests compare with -- against networkx'
weakly_connected_components on small graphs, one of them a karate train split."""
import networkx as nx
import numpy as np
import pytest

import lcc_refs


def nx_lcc(n, src, dst):
    """Labels, winner and kept nodes from networkx alone: components in node order 0..n-1, max(..., key=len) as the reference picks."""
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    G.add_edges_from(zip(np.asarray(src).tolist(), np.asarray(dst).tolist()))
    comps = list(nx.weakly_connected_components(G))
    labels = np.empty(n, np.int32)
    for c in comps:
        labels[list(c)] = min(c)
    big = max(comps, key=len)                                  # the first maximum, components found in node order
    return len(comps), labels, sorted(big)


def small_graphs():
    rng = np.random.RandomState(3)
    out = {'two_triangles_tie': (6, [3, 4, 5, 0, 1, 2], [4, 5, 3, 1, 2, 0]),
           'one_way_chain': (7, [6, 4, 2, 1], [4, 2, 1, 1]),
           'no_arcs': (5, [], []),
           'single': (1, [0], [0])}
    for k in range(4):
        n = 40 + 7 * k
        m = 25 + 5 * k
        out['random%d' % k] = (n, rng.randint(0, n, m), rng.randint(0, n, m))
    return out


@pytest.mark.parametrize('name', sorted(small_graphs()))
def test_restatement_equals_networkx(name):
    n, src, dst = small_graphs()[name]
    src = np.asarray(src, np.int32); dst = np.asarray(dst, np.int32)
    ncomp, labels, big = nx_lcc(n, src, dst)
    got_n, got_labels = lcc_refs.cc_labels(n, src, dst)
    assert got_n == ncomp and np.array_equal(got_labels, labels)
    r = lcc_refs.lcc(n, src, dst, np.arange(len(src), dtype=np.float32))
    assert r['old_of_new'].tolist() == big and r['winner'] == big[0]
    assert np.array_equal(r['new_of_old'][r['old_of_new']], np.arange(len(big)))
    assert (r['new_of_old'] >= 0).sum() == len(big)
    inside = np.isin(src, big)
    assert np.array_equal(r['old_of_new'][r['src']], src[inside]) and np.array_equal(r['old_of_new'][r['dst']], dst[inside])      # order kept
    assert np.array_equal(r['w'], np.flatnonzero(inside).astype(np.float32))


@pytest.mark.parametrize('ratio,arcs,ncomp,largest', [(0.5, 41, 6, 27), (0.2, None, 23, None)])
def test_karate_train_split(karate, ratio, arcs, ncomp, largest):
    train, test = lcc_refs.karate_train_split(karate, ratio)
    want_n, labels, big = nx_lcc(train.n, train.src, train.dst)
    r = lcc_refs.lcc(train.n, train.src, train.dst, train.w)
    assert r['n_components'] == want_n == ncomp
    assert np.array_equal(r['labels'], labels) and r['old_of_new'].tolist() == big
    if arcs is not None:
        assert train.number_of_edges() == arcs and len(big) == largest
    # the subgraph networkx cuts out has exactly the arcs the restatement keeps
    G = train.to_networkx().subgraph(big)
    assert sorted(G.edges()) == sorted(zip(r['old_of_new'][r['src']].tolist(), r['old_of_new'][r['dst']].tolist()))
    s, d = lcc_refs.restrict_test(r['new_of_old'], test.src, test.dst)
    keep = np.isin(test.src, big) & np.isin(test.dst, big)
    assert np.array_equal(r['old_of_new'][s], test.src[keep]) and np.array_equal(r['old_of_new'][d], test.dst[keep])
