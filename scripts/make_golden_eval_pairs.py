#!/usr/bin/env python3
"""Generate tests/golden/eval_pairs_ref.json by RUNNING THE REFERENCE's pair-sampled evaluator (in the manner of make_golden.py).

Run once where the reference checkout exists:  python scripts/make_golden_eval_pairs.py
The output is a data fixture; the tests never need the reference.

What is executed, from the reference:
  gem/utils/evaluation_util.py:20-26     get_edge_list_from_adj_mtrx(adj, is_undirected=..., edge_pairs=[...])   (adj >= 0)
  gem/evaluation/metrics.py:27-46, 6-24  computeMAP, computePrecisionCurve
  static_graph_embedding.py:48-65        get_reconstructed_adj: the method's own get_edge_weight loop (gf.py:103, hope.py:43, lap.py:74,
                                         lle.py:53) over X cast to fp32 and back to fp64 -- the inputs the device kernel sees
i.e. evaluate_graph_reconstruction.py:14-36 with an EXPLICIT pair list in place of get_random_edge_pairs, which draws from `secrets` and
cannot be reproduced.  The pair lists are drawn here with numpy and recorded in the fixture; a self-pair and (for the inner-product
cases that have one) a pair with a negative score are appended by hand when the draw has none.

The weighted branch (evaluate_graph_reconstruction.py:38-42) calls nx.to_numpy_matrix, which networkx 3 no longer has; lines 39-42 are
RESTATED here with nx.to_numpy_array on a weighted copy of karate whose nodes are inserted in id order (the matrix rows then follow the
node ids, as the reconstructed matrix does).

Cases: karate (n = 34), ratio 0.3, undirected and directed, the four committed reference embeddings; sbm1024, ratio 0.01 (5 238 pairs),
gf_sbm1024_d32 / hope_sbm1024_d32 and one coarse-grid embedding round(2 randn)/2, d = 4, whose scores tie exactly.
"""
import json
import os
import sys

REF = '/root/reference'
sys.path.insert(0, REF)
os.environ.setdefault('MPLBACKEND', 'Agg')

import numpy as np
import networkx as nx

if not hasattr(nx, 'to_numpy_matrix'):          # removed in networkx 3; the embedding modules import-time reference it
    nx.to_numpy_matrix = lambda g, *a, **k: np.asmatrix(nx.to_numpy_array(g, *a, **k))

from gem.utils import graph_util                                       # noqa: E402
from gem.utils.evaluation_util import get_edge_list_from_adj_mtrx     # noqa: E402
from gem.evaluation.metrics import computeMAP, computePrecisionCurve  # noqa: E402
from gem.embedding.gf import GraphFactorization                        # noqa: E402
from gem.embedding.hope import HOPE                                    # noqa: E402
from gem.embedding.lap import LaplacianEigenmaps                       # noqa: E402
from gem.embedding.lle import LocallyLinearEmbedding                   # noqa: E402

OUT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))


def load_karate():
    return graph_util.loadGraphFromEdgeListTxt(os.path.join(OUT, 'karate.edgelist'), directed=True).to_directed()


def load_sbm():
    G = nx.DiGraph()
    G.add_nodes_from(np.load(os.path.join(OUT, 'sbm1024_nodes.npy')).tolist())
    G.add_edges_from(map(tuple, np.load(os.path.join(OUT, 'sbm1024_edges.npy')).tolist()))
    return G


def draw_pairs(n, ratio, undirected, seed):
    """The reference's count (evaluation_util.py:6-10) of distinct pairs, no pair together with its reverse when undirected."""
    num = int(ratio * n * (n - 1))
    if undirected:
        num = num / 2
    rng = np.random.RandomState(seed)
    cur, out = set(), []
    while len(cur) < num:
        p = (int(rng.randint(n)), int(rng.randint(n)))
        if p in cur or (undirected and (p[1], p[0]) in cur):
            continue
        cur.add(p)
        out.append(p)
    return out


def add_by_hand(pairs, undirected, candidates):
    for p in candidates:
        p = (int(p[0]), int(p[1]))
        if p in pairs or (undirected and (p[1], p[0]) in pairs):
            continue
        pairs.append(p)
        return True
    return False


def recon(model, X):
    X32 = np.asarray(X).astype(np.float32).astype(np.float64)
    return np.asarray(model.get_reconstructed_adj(X32))


def main():
    kar, sbm = load_karate(), load_sbm()
    emb = {
        'karate_gf': (GraphFactorization(d=2, max_iter=1, eta=1e-4, regu=1.0, data_set='golden'), 'ref_karate_GraphFactorization.txt'),
        'karate_hope': (HOPE(d=4, beta=0.01), 'ref_karate_HOPE.txt'),
        'karate_lap': (LaplacianEigenmaps(d=2), 'ref_karate_LaplacianEigenmaps.txt'),
        'karate_lle': (LocallyLinearEmbedding(d=2), 'ref_karate_LocallyLinearEmbedding.txt'),
        'sbm1024_gf': (GraphFactorization(d=32, max_iter=1, eta=0.02, regu=0.01, data_set='golden'), 'gf_sbm1024_d32.npz'),
        'sbm1024_hope': (HOPE(d=32, beta=0.01), 'hope_sbm1024_d32.npz'),
        'sbm1024_grid': (GraphFactorization(d=4, max_iter=1, eta=0.1, regu=0.1, data_set='golden'), None),
    }
    adj = {}
    for key, (model, f) in emb.items():
        if f is None:
            X = np.round(np.random.RandomState(0).randn(1024, 4) * 2) / 2
        elif f.endswith('.npz'):
            X = np.load(os.path.join(OUT, f))['X']
        else:
            X = np.loadtxt(os.path.join(OUT, f))
        adj[key] = recon(model, X)
        print(key, X.shape, 'negative scores:', int((adj[key] < 0).sum()), flush=True)

    inner = {'karate': ('karate_gf', 'karate_hope'), 'sbm1024': ('sbm1024_gf', 'sbm1024_hope', 'sbm1024_grid')}
    lists = {}
    for gname, n, ratio, modes in (('karate', 34, 0.3, (True, False)), ('sbm1024', 1024, 0.01, (True,))):
        for und in modes:
            pairs = draw_pairs(n, ratio, und, seed=7 + n + int(und))
            if not any(a == b for a, b in pairs):
                add_by_hand(pairs, und, [(5, 5)])
            for key in inner[gname]:
                if not any(adj[key][a, b] < 0 for a, b in pairs):
                    neg = np.argwhere(adj[key] < 0)
                    print('  %s: no negative score drawn; appended by hand: %s' % (key, add_by_hand(pairs, und, neg) if len(neg) else 'none exists'))
            lists['%s_%s' % (gname, 'undirected' if und else 'directed')] = pairs

    cases = []
    for key, (model, f) in emb.items():
        gname = key.split('_')[0]
        G = kar if gname == 'karate' else sbm
        for und in ((True, False) if gname == 'karate' else (True,)):
            lname = '%s_%s' % (gname, 'undirected' if und else 'directed')
            pairs = lists[lname]
            el = get_edge_list_from_adj_mtrx(adj[key], is_undirected=und, edge_pairs=pairs)
            MAP = computeMAP(el, G, is_undirected=und)
            prec, _ = computePrecisionCurve(el, G)
            cases.append({'name': '%s_%s' % (key, 'undirected' if und else 'directed'), 'graph': gname, 'method': key.split('_')[1],
                          'embedding': f, 'pairs': lname, 'is_undirected': und, 'kept_pairs': len(el), 'MAP': float(MAP),
                          'prec_curv': [float(p) for p in prec]})
            print(cases[-1]['name'], len(pairs), len(el), MAP, flush=True)

    # ---- weighted error: evaluate_graph_reconstruction.py:39-42 restated (see the module docstring)
    W = nx.DiGraph()
    W.add_nodes_from(range(34))
    wedges = [(i, j, 0.5 + 0.25 * ((7 * i + 3 * j) % 5)) for i, j in kar.edges()]            # exactly representable in fp32
    W.add_weighted_edges_from(wedges)
    weighted = {'edges': wedges, 'cases': []}
    for key in ('karate_gf', 'karate_hope', 'karate_lap', 'karate_lle'):
        digraph_adj = nx.to_numpy_array(W)
        estimated_adj = adj[key].copy()
        estimated_adj[digraph_adj == 0] = 0
        err = np.linalg.norm(digraph_adj - estimated_adj)
        err_baseline = np.linalg.norm(digraph_adj)
        weighted['cases'].append({'method': key.split('_')[1], 'embedding': emb[key][1], 'err': float(err), 'err_baseline': float(err_baseline)})
        print(key, err, err_baseline)

    path = os.path.join(OUT, 'eval_pairs_ref.json')
    with open(path, 'w') as f:
        json.dump({'pairs': lists, 'cases': cases, 'weighted': weighted}, f, separators=(',', ':'))
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
