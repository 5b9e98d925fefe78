"""Writes tests/golden/link_baselines_ref.json: the neighbourhood link-prediction baselines on the SBM-1024 link fixture, from networkx and
sklearn.  CPU only; needs networkx and scikit-learn (3.4.2 and 1.7.2 when the fixture was made).

    python scripts/make_golden_link_baselines.py

Per heuristic (cn, jaccard, aa, ra, pa), for the fixture's test pairs (tests/rank_refs.py fixture_pairs()) scored on the TRAIN graph by
networkx's common_neighbors, jaccard_coefficient, adamic_adar_index, resource_allocation_index and preferential_attachment on an nx.Graph:
sklearn's roc_auc_score and average_precision_score, the number of distinct scores, and how far sklearn's two figures are from the exact
rationals.  For aa and ra, whose sums depend on the order of addition: delta = 4 x the largest score tolerance (k + 1) 2^-53 score over the
pairs (k common neighbours; a device score and networkx's each lie within one tolerance of the correctly rounded sum, so a difference of two
scores moves by at most four), `near` = the (positive, negative) pairs whose scores lie within delta, and the AP sensitivity at delta, as
scripts/make_golden_link_auc.py computes them.  Inputs are NOT stored: rank_refs rebuilds them from sbm1024_edges.npy and seeds."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
HEURISTICS = ('cn', 'jaccard', 'aa', 'ra', 'pa')


def train_nx_graph(train):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(train.n))
    G.add_edges_from((int(a), int(b)) for a, b in zip(train.src.tolist(), train.dst.tolist()) if a != b)
    return G


def networkx_scores(G, st, ed):
    """{name: float64 (m,)} by networkx's own functions, pair by pair."""
    import networkx as nx
    pairs = list(zip(np.asarray(st).tolist(), np.asarray(ed).tolist()))
    out = {'cn': np.array([len(list(nx.common_neighbors(G, u, v))) for u, v in pairs], dtype=np.float64)}
    for name, fn in (('jaccard', nx.jaccard_coefficient), ('aa', nx.adamic_adar_index), ('ra', nx.resource_allocation_index),
                     ('pa', nx.preferential_attachment)):
        out[name] = np.array([s for _, _, s in fn(G, pairs)], dtype=np.float64)
    return out


def report():
    import networkx
    import sklearn
    from sklearn.metrics import average_precision_score, roc_auc_score
    import rank_refs as R
    train, _, pairs = R.fixture_pairs()
    st, ed, y = pairs['test']
    score = networkx_scores(train_nx_graph(train), st, ed)
    out = {'sklearn': sklearn.__version__, 'networkx': networkx.__version__, 'heuristics': {}}
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        out[k] = int(pairs[k])
    for name in HEURISTICS:
        s = score[name]
        ex = R.exact_scores(s, y)
        auc, ap = float(roc_auc_score(y, s)), float(average_precision_score(y, s))
        entry = {'auc': auc, 'ap': ap, 'n_thresholds': ex['T'], 'sklearn_vs_exact': max(abs(auc - float(ex['auc'])), abs(ap - float(ex['ap'])))}
        if name in ('aa', 'ra'):
            delta = 4 * float(((score['cn'] + 1.0) * 2.0 ** -53 * s).max())
            near = R.near_pairs(s, y, delta)
            entry.update({'delta': delta, 'near': near, 'near_share': near / float(ex['P'] * ex['N']), 'ap_sensitivity': R.ap_sensitivity(s, y, delta)})
        out['heuristics'][name] = entry
    return out


def main():
    rep = report()
    for name in HEURISTICS:
        print(name, json.dumps(rep['heuristics'][name]))
    with open(os.path.join(GOLDEN, 'link_baselines_ref.json'), 'w') as f:
        json.dump(rep, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
