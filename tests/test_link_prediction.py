"""CPU tier of link prediction (gem_amd/evaluation/link_prediction.py) against tests/golden/linkpred_ref.json, which
scripts/make_golden_linkpred.py produced by running the reference's split_di_graph_to_train_test, get_edge_list_from_adj_mtrx, the literal
`not train.has_edge(st, ed)` filter, computeMAP and computePrecisionCurve: MAP, every node's AP and prec_curv element by element to 1e-12
(prec_curv of sbm1024 is recorded as its first 256 entries, its length and its sum; the arrays are in linkpred_ref.npz).  The grid embedding's scores tie exactly: there the
recorded prec_curv entries -- quotients of two integers, so a function of the ORDER alone -- must be reproduced bit for bit."""
import json

import numpy as np
import pytest

from gem_amd.embedding.static_graph_embedding import StaticGraphEmbedding
from gem_amd.evaluation import link_prediction as lp
from gem_amd.evaluation import reconstruction as gr
from gem_amd.graph import EdgeListGraph
from conftest import golden_path
from test_eval_pairs import embedding_of, model_of

REF = json.load(open(golden_path('linkpred_ref.json')))           # the index; the arrays (split bits, per-node AP, prec_curv) are in the .npz
ARR = np.load(golden_path('linkpred_ref.npz'))
CASES = {c['name']: dict(c, ap=ARR[c['name'] + '/ap'], prec_curv=ARR[c['name'] + '/prec_curv'].tolist()) for c in REF['cases']}


def graph_of(split, karate, sbm1024):
    if split['graph'] == 'karate_sym':                               # karate's symmetric closure, edge list recorded by the fixture
        import networkx as nx
        G = nx.DiGraph()
        G.add_nodes_from(karate.nodes)
        G.add_edges_from(map(tuple, ARR['karate_sym_edges'].tolist()))
        return G
    return karate if split['graph'] == 'karate' else sbm1024


def truths_of(sname, G):
    """Dense train / test adjacency from the recorded bits over list(G.edges())."""
    e = np.array(list(G.edges()))
    assert len(e) == REF['splits'][sname]['edges']
    n = len(G.nodes)
    out = []
    for tag in ('train_bits', 'test_bits'):
        on = np.unpackbits(ARR[sname + '/' + tag])[:len(e)].astype(bool)
        t = np.zeros((n, n), dtype=bool); t[e[on, 0], e[on, 1]] = True
        out.append(t)
    return out


def case_inputs(c, karate, sbm1024):
    split = REF['splits'][c['split']]
    G = graph_of(split, karate, sbm1024)
    train, test = truths_of(c['split'], G)
    cc = dict(c, graph=split['graph'].split('_')[0])
    return G, split, model_of(cc).get_reconstructed_adj(embedding_of(cc)), train, test


def test_fixture_covers_what_the_issue_lists():
    assert len(CASES) == 28
    for fam, count in (('karate_gf', 4), ('karate_hope', 4), ('karate_lap', 4), ('karate_lle', 4), ('sbm1024_gf', 4), ('sbm1024_hope', 4), ('sbm1024_grid', 4)):
        names = [nm for nm in CASES if nm.startswith(fam + '_')]
        assert len(names) == count and {CASES[nm]['is_undirected'] for nm in names} == {True, False}
        assert {REF['splits'][CASES[nm]['split']]['train_ratio'] for nm in names} == {0.8, 0.5}
    for c in CASES.values():
        assert len(c['prec_curv']) == min(c['prec_len'], 256 if c['prec_len'] > 1200 else c['prec_len'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_dense_link_prediction_reproduces_the_reference(name, karate, sbm1024):
    c = CASES[name]
    G, split, score, train, test = case_inputs(c, karate, sbm1024)
    und = c['is_undirected']
    ap = lp.link_prediction_rows(score, train, test, undirected=und)
    MAP, prec = lp.link_prediction_dense(score, train, test, und)
    print('%s: |MAP - ref| = %.3g, max |AP - ref| = %.3g' % (name, abs(MAP - c['MAP']), np.abs(ap - np.array(c['ap'])).max()))
    assert abs(MAP - c['MAP']) <= 1e-12
    assert np.all(np.abs(ap - np.array(c['ap'])) <= 1e-12)
    assert len(prec) == c['prec_len']
    head = np.array(prec[:len(c['prec_curv'])])
    assert np.all(np.abs(head - np.array(c['prec_curv'])) <= 1e-12)
    # the whole curve through its sum: both sides add prec_len numbers in [0, 1] left to right, each addition rounding by at most 2^-53 of the sum
    assert abs(np.cumsum(prec)[-1] - c['prec_sum']) <= 2 * c['prec_len'] * 2.0 ** -53 * c['prec_sum']
    if c['method'] == 'grid':                                        # exact ties everywhere: the id order decides, and decides the same way
        assert prec[:len(c['prec_curv'])] == c['prec_curv']
        assert lp.link_prediction_dense(score, train, test, und, max_k=100)[1] == prec[:100]
    # a train arc never ranks: scoring it highest changes nothing
    boosted = score.copy(); boosted[train] = 1e9
    assert np.array_equal(lp.link_prediction_rows(boosted, train, test, undirected=und), ap)


def test_unfiltered_ranking_differs(karate):
    """What the mask is for: without the filter the same embedding scores differently (the training arcs take the top ranks)."""
    c = CASES['karate_gf_directed_0.8']
    _, _, score, train, test = case_inputs(c, karate, None)
    assert abs(lp.link_prediction_dense(score, np.zeros_like(train), test, False)[0] - c['MAP']) > 1e-3


@pytest.mark.parametrize('sname', sorted(REF['splits']))
def test_pairs_filter_equals_has_edge(sname, karate, sbm1024):
    split = REF['splits'][sname]
    G = graph_of(split, karate, sbm1024)
    train, _ = truths_of(sname, G)
    n = train.shape[0]
    rng = np.random.RandomState(5)
    ts, td = np.nonzero(train)
    st = np.concatenate([rng.randint(0, n, 3000), ts[:200], td[:200], [0, n - 1]])
    ed = np.concatenate([rng.randint(0, n, 3000), td[:200], ts[:200], [0, n - 1]])
    keep = lp.pairs_not_in_train(n, st, ed, ts, td)
    assert np.array_equal(keep, ~train[st, ed]) and not keep[3000:3000 + min(200, len(ts))].any()          # (the train arcs themselves go)
    assert lp.pairs_not_in_train(n, st, ed, ts[:0], td[:0]).all()


class FixedEmbedding(StaticGraphEmbedding):
    """A model that 'learns' a table it was given: the whole evaluateStaticLinkPrediction path without a device."""
    hyper_params = {'method_name': 'graph_factor_sgd'}

    def __init__(self, X):
        super(FixedEmbedding, self).__init__(d=X.shape[1])
        self._fixed, self.trained_on = X, None

    def learn_embedding(self, graph=None, **_ignored):
        self.trained_on = graph
        self._X = self._fixed
        return self._X


@pytest.mark.parametrize('name', ['karate_gf_directed_0.8', 'karate_gf_undirected_0.5'])
def test_evaluate_static_link_prediction_end_to_end(name, karate):
    c = CASES[name]
    split = REF['splits'][c['split']]
    G = graph_of(split, karate, None)
    train, _ = truths_of(c['split'], G)
    model = FixedEmbedding(embedding_of(dict(c, graph='karate')))
    np.random.seed(split['seed'])
    MAP, prec = lp.evaluateStaticLinkPrediction(G, model, train_ratio=split['train_ratio'], is_undirected=c['is_undirected'])
    assert np.array_equal(gr._adjacency_bool(model.trained_on, 34), train)          # it trained on the reference's train graph of that seed
    assert abs(MAP - c['MAP']) <= 1e-12
    assert len(prec) == c['prec_len'] and np.all(np.abs(np.array(prec) - np.array(c['prec_curv'])) <= 1e-12)


def test_dense_path_refuses_large_graphs_without_sampling():
    g = EdgeListGraph(lp.DENSE_MAX_N + 1, [0, 1], [1, 0])
    model = FixedEmbedding(np.zeros((lp.DENSE_MAX_N + 1, 2)))
    with pytest.raises(ValueError, match='dense limit of 4096.*`nodes`.*`sample_ratio_e`'):
        lp.evaluateStaticLinkPrediction(g, model)
    assert model.trained_on is None                                  # refused before any training


def test_alias_imports():
    from gem.evaluation import evaluate_link_prediction as alias
    assert alias.evaluateStaticLinkPrediction is lp.evaluateStaticLinkPrediction
    assert alias.evaluate_link_prediction_gpu is lp.evaluate_link_prediction_gpu
