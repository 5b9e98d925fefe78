"""Pair-sampled graph reconstruction (the reference's `sample_ratio_e`) on the host: random_edge_pairs, pair_metrics and
evaluateStaticGraphReconstruction(edge_pairs=...) against tests/golden/eval_pairs_ref.json, which scripts/make_golden_eval_pairs.py
produced with the reference's get_edge_list_from_adj_mtrx / computeMAP / computePrecisionCurve
(evaluate_graph_reconstruction.py:8-46, evaluation_util.py:5-36, metrics.py:6-46)."""
import json
import math

import numpy as np
import pytest

from gem_amd.embedding.gf import GraphFactorization
from gem_amd.embedding.hope import HOPE
from gem_amd.embedding.lap import LaplacianEigenmaps
from gem_amd.embedding.lle import LocallyLinearEmbedding
from gem_amd.evaluation import reconstruction as gr
from conftest import golden_path

REF = json.load(open(golden_path('eval_pairs_ref.json')))
CASES = {c['name']: c for c in REF['cases']}


def model_of(case):
    d = {'karate': {'gf': 2, 'hope': 4, 'lap': 2, 'lle': 2}, 'sbm1024': {'gf': 32, 'hope': 32, 'grid': 4}}[case['graph']][case['method']]
    return {'gf': lambda: GraphFactorization(d=d, max_iter=1, eta=0.02, regu=0.01), 'grid': lambda: GraphFactorization(d=d, max_iter=1, eta=0.1, regu=0.1),
            'hope': lambda: HOPE(d=d, beta=0.01), 'lap': lambda: LaplacianEigenmaps(d=d), 'lle': lambda: LocallyLinearEmbedding(d=d)}[case['method']]()


def embedding_of(case):
    f = case['embedding']
    if f is None:
        X = np.round(np.random.RandomState(0).randn(1024, 4) * 2) / 2
    elif f.endswith('.npz'):
        X = np.load(golden_path(f))['X']
    else:
        X = np.loadtxt(golden_path(f))
    return np.asarray(X).astype(np.float32).astype(np.float64)               # the fixture scores the fp32-rounded embedding


def scalar_scores(model, X, st, ed):
    """get_edge_weight pair by pair (the reference's definition), zero on the diagonal."""
    model._X = X
    return np.array([0.0 if a == b else float(model.get_edge_weight(a, b)) for a, b in zip(st, ed)])


def weighted_karate():
    import networkx as nx
    G = nx.DiGraph()
    G.add_nodes_from(range(34))
    G.add_weighted_edges_from([tuple(e) for e in REF['weighted']['edges']])
    return G


def test_fixture_holds_the_edge_cases_the_metric_must_get_right():
    for name, pairs in REF['pairs'].items():
        assert any(a == b for a, b in pairs), name
    for c in REF['cases']:
        if c['method'] in ('gf', 'hope', 'grid'):
            assert c['kept_pairs'] < len(REF['pairs'][c['pairs']]), c['name']   # some pair scored < 0 and was dropped
        assert len(c['prec_curv']) == c['kept_pairs']


@pytest.mark.parametrize('name', sorted(CASES))
def test_pair_metrics_reproduces_the_reference(name, karate, sbm1024):
    c = CASES[name]
    G = karate if c['graph'] == 'karate' else sbm1024
    n = len(G.nodes)
    pairs = np.array(REF['pairs'][c['pairs']])
    st, ed = pairs[:, 0], pairs[:, 1]
    score = scalar_scores(model_of(c), embedding_of(c), st, ed)
    truth = gr._adjacency_bool(G, n)
    MAP, prec = gr.pair_metrics(n, st, ed, score, truth[st, ed], c['is_undirected'], out_degree=truth.sum(axis=1))
    assert abs(MAP - c['MAP']) <= 1e-12
    assert prec == c['prec_curv']


@pytest.mark.parametrize('name', sorted(CASES))
def test_evaluator_with_edge_pairs_reproduces_the_reference(name, karate, sbm1024):
    c = CASES[name]
    G = karate if c['graph'] == 'karate' else sbm1024
    MAP, prec, err, base = gr.evaluateStaticGraphReconstruction(G, model_of(c), embedding_of(c), None, is_undirected=c['is_undirected'],
                                                                edge_pairs=REF['pairs'][c['pairs']])
    assert abs(MAP - c['MAP']) <= 1e-12
    if c['method'] == 'grid':
        assert MAP == c['MAP']               # exact scores, and pair_metrics adds in the reference's order
    assert prec == c['prec_curv']
    assert err is None and base is None


@pytest.mark.parametrize('k', range(len(REF['weighted']['cases'])))
def test_weighted_error_with_edge_pairs(k):
    w = REF['weighted']['cases'][k]
    c = CASES['karate_%s_undirected' % w['method']]
    _, _, err, base = gr.evaluateStaticGraphReconstruction(weighted_karate(), model_of(c), embedding_of(c), None, is_weighted=True,
                                                           edge_pairs=REF['pairs'][c['pairs']])
    assert abs(err - w['err']) <= 1e-12 * w['err']
    assert abs(base - w['err_baseline']) <= 1e-12 * w['err_baseline']


@pytest.mark.parametrize('n,ratio', [(34, 0.3), (1024, 0.01), (7, 1.0)])
@pytest.mark.parametrize('undirected', [True, False])
def test_random_edge_pairs_counts_and_distinctness(n, ratio, undirected):
    num = int(ratio * n * (n - 1))                                   # evaluation_util.py:6-10: while len(set) < num_pairs (/ 2 as a float)
    want = math.ceil(num / 2) if undirected else num
    p = gr.random_edge_pairs(n, ratio, undirected, seed=3)
    assert p.shape == (want, 2) and p.min() >= 0 and p.max() < n
    as_set = set(map(tuple, p.tolist()))
    assert len(as_set) == want                                       # no duplicates
    if undirected:
        assert not any(a != b and (b, a) in as_set for a, b in as_set)
    assert np.array_equal(p, gr.random_edge_pairs(n, ratio, undirected, seed=3))
    assert not np.array_equal(p, gr.random_edge_pairs(n, ratio, undirected, seed=4))
    if n == 7 and not undirected:
        assert want == 42                                            # all ordered pairs of distinct nodes fit; self-pairs may take their place


def test_sample_ratio_e_no_longer_raises(karate):
    m = GraphFactorization(d=2, max_iter=1, eta=1e-4, regu=1.0)
    X = np.loadtxt(golden_path('ref_karate_GraphFactorization.txt'))
    out = gr.evaluateStaticGraphReconstruction(karate, m, X, None, sample_ratio_e=0.3)
    again = gr.evaluateStaticGraphReconstruction(karate, m, X, None, sample_ratio_e=0.3)
    other = gr.evaluateStaticGraphReconstruction(karate, m, X, None, sample_ratio_e=0.3, seed=1)
    assert 0.0 <= out[0] <= 1.0 and 0 < len(out[1]) <= 168
    assert out == again and out[1] != other[1]
    full = gr.evaluateStaticGraphReconstruction(karate, m, X, None)            # the all-pairs path is untouched
    assert len(full[1]) > 168


def test_new_names_are_exported_next_to_the_evaluator():
    from gem.evaluation import evaluate_graph_reconstruction as alias
    for name in ('evaluateStaticGraphReconstruction', 'evaluate_reconstruction_gpu', 'pair_metrics', 'random_edge_pairs', 'sampled_ap_gpu'):
        assert getattr(alias, name) is getattr(gr, name)


def test_pair_metrics_directed_needs_out_degree():
    with pytest.raises(ValueError):
        gr.pair_metrics(3, [0], [1], [1.0], [True], is_undirected=False)
