#!/usr/bin/env python3
"""Generate tests/golden/linkpred_ref.json and linkpred_ref.npz by RUNNING THE REFERENCE's functions (in the manner of make_golden_eval_pairs.py).

Run once where the reference checkout exists:  python scripts/make_golden_linkpred.py [reference checkout]
The output is a data fixture; the tests never need the reference.

What is executed, from the reference:
  gem/utils/evaluation_util.py:39-53     split_di_graph_to_train_test under np.random.seed(seed)
  static_graph_embedding.py:48-65        get_reconstructed_adj: the method's own get_edge_weight loop over X cast to fp32 and back to fp64
  gem/utils/evaluation_util.py:20-36     get_edge_list_from_adj_mtrx(adj, is_undirected=...)          (all pairs, adj > 0)
  [e for e in edge_list if not train.has_edge(e[0], e[1])]                                            the train filter, literally
  gem/evaluation/metrics.py:27-46, 6-24  computeMAP, computePrecisionCurve against the TEST graph
The per-node AP is computeMAP of one node's edges alone, with is_undirected=True so that every node counts, times the node count.

The reference's undirected split removes (ed, st) with every (st, ed) and raises on karate.edgelist, which lists every edge one way only:
the undirected karate cases run on its symmetric closure G.to_undirected().to_directed(), whose edge list is recorded ('karate_sym').

Cases: karate with the four committed reference embeddings; sbm1024 with gf_sbm1024_d32, hope_sbm1024_d32 and one coarse-grid embedding
round(2 randn)/2, d = 4, whose scores tie exactly.  Each runs undirected and directed, at train_ratio 0.8 and 0.5.

Two files: linkpred_ref.json is the index (per split: graph, mode, train_ratio, seed, edge count; per case: MAP, the length of prec_curv and its
sum in the reference's order, left to right), linkpred_ref.npz holds the arrays (float64 / uint8, so that the fixture stays small):
  '<split>/train_bits', '<split>/test_bits'   over list(G.edges()), which edges the train and the test graph hold (one bit per edge, np.packbits)
  '<case>/ap'                                 every node's AP
  '<case>/prec_curv'                          prec_curv, whole when it has at most 1200 entries, else its first 256 entries
  'karate_sym_edges'                          the edge list of karate's symmetric closure
"""
import json
import os
import sys

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('GEM_REFERENCE')
if not REF:
    sys.exit('usage: make_golden_linkpred.py <reference checkout>   (or GEM_REFERENCE in the environment)')
sys.path.insert(0, REF)
os.environ.setdefault('MPLBACKEND', 'Agg')

import numpy as np
import networkx as nx

if not hasattr(nx, 'to_numpy_matrix'):          # removed in networkx 3; the embedding modules import-time reference it
    nx.to_numpy_matrix = lambda g, *a, **k: np.asmatrix(nx.to_numpy_array(g, *a, **k))

from gem.utils import graph_util                                                                   # noqa: E402
from gem.utils.evaluation_util import get_edge_list_from_adj_mtrx, split_di_graph_to_train_test    # noqa: E402
from gem.evaluation.metrics import computeMAP, computePrecisionCurve                               # noqa: E402
from gem.embedding.gf import GraphFactorization                                                    # noqa: E402
from gem.embedding.hope import HOPE                                                                # noqa: E402
from gem.embedding.lap import LaplacianEigenmaps                                                   # noqa: E402
from gem.embedding.lle import LocallyLinearEmbedding                                               # noqa: E402

OUT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden'))
PREC_WHOLE, PREC_HEAD = 1200, 256


def load_karate():
    return graph_util.loadGraphFromEdgeListTxt(os.path.join(OUT, 'karate.edgelist'), directed=True).to_directed()


def load_sbm():
    G = nx.DiGraph()
    G.add_nodes_from(np.load(os.path.join(OUT, 'sbm1024_nodes.npy')).tolist())
    G.add_edges_from(map(tuple, np.load(os.path.join(OUT, 'sbm1024_edges.npy')).tolist()))
    return G


def recon(model, X):
    X32 = np.asarray(X).astype(np.float32).astype(np.float64)
    return np.asarray(model.get_reconstructed_adj(X32))


def bits(flags):
    return np.packbits(np.asarray(flags, dtype=bool))


def main():
    kar = load_karate()
    graphs = {'karate': kar, 'karate_sym': kar.to_undirected().to_directed(), 'sbm1024': load_sbm()}
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
        print(key, X.shape, flush=True)

    splits, cases, arrays = {}, [], {'karate_sym_edges': np.array(list(graphs['karate_sym'].edges()), dtype=np.int64)}
    for gname, G in graphs.items():
        n = len(G.nodes)
        edges = list(G.edges())
        for und in {'karate': (False,), 'karate_sym': (True,)}.get(gname, (True, False)):
            for ratio in (0.8, 0.5):
                sname = '%s_%s_%g' % (gname, 'undirected' if und else 'directed', ratio)
                seed = 1000 + len(splits)
                np.random.seed(seed)
                train, test = split_di_graph_to_train_test(G, ratio, is_undirected=und)
                splits[sname] = {'graph': gname, 'is_undirected': und, 'train_ratio': ratio, 'seed': seed, 'edges': len(edges)}
                arrays[sname + '/train_bits'] = bits([train.has_edge(a, b) for a, b in edges])
                arrays[sname + '/test_bits'] = bits([test.has_edge(a, b) for a, b in edges])
                both = sum(1 for a, b in edges if train.has_edge(a, b) and test.has_edge(a, b))
                print(sname, 'train', train.number_of_edges(), 'test', test.number_of_edges(), 'in both', both, flush=True)
                for key in [k for k in emb if k.startswith(gname.split('_')[0] + '_')]:
                    el = get_edge_list_from_adj_mtrx(adj[key], is_undirected=und)
                    el = [e for e in el if not train.has_edge(e[0], e[1])]
                    MAP = computeMAP(el, test, is_undirected=und)
                    prec, _ = computePrecisionCurve(el, test)
                    by_node = [[] for _ in range(n)]
                    for e in el:
                        by_node[e[0]].append(e)
                    ap = [float(computeMAP(by_node[i], test, is_undirected=True) * n) if by_node[i] else 0.0 for i in range(n)]
                    case = {'name': '%s_%s_%g' % (key, 'undirected' if und else 'directed', ratio), 'split': sname, 'method': key.split('_')[1],
                            'embedding': emb[key][1], 'is_undirected': und, 'MAP': float(MAP), 'prec_len': len(prec), 'prec_sum': float(sum(prec))}
                    arrays[case['name'] + '/ap'] = np.array(ap, dtype=np.float64)
                    arrays[case['name'] + '/prec_curv'] = np.array(prec if len(prec) <= PREC_WHOLE else prec[:PREC_HEAD], dtype=np.float64)
                    cases.append(case)
                    print(' ', case['name'], 'candidates', len(el), 'MAP', MAP, flush=True)

    path = os.path.join(OUT, 'linkpred_ref.json')
    with open(path, 'w') as f:
        f.write('{"splits": {\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(v)) for k, v in splits.items()) + '\n},\n"cases": [\n' +
                ',\n'.join(' ' + json.dumps(c) for c in cases) + '\n]}\n')             # one split, one case per line
    print(path, os.path.getsize(path), 'bytes')
    path = os.path.join(OUT, 'linkpred_ref.npz')
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
