"""Link prediction as classification on the SBM-1024 fixture graph on the GPU -- the protocol of the node2vec paper's table 4: hold out 20 %
of the edges, embed the rest with HOPE, turn node pairs into features with the four binary operators, fit a logistic regression on the
training pairs and report ROC-AUC and average precision on the held-out edges against as many non-edges.  'dot' ranks by the inner product
without a classifier, 'method' by HOPE's own edge weight.  Three seeded rounds each.

    python examples/run_sbm_link_auc_hip.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gem_amd.embedding.hope import HOPE                                          # noqa: E402
from gem_amd.evaluation.link_classification import FEATURE_OPS, expLinkClassification   # noqa: E402
from gem_amd.graph import EdgeListGraph                                          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def main():
    edges = np.load(os.path.join(GOLDEN, 'sbm1024_edges.npy'))
    graph = EdgeListGraph(1024, edges[:, 0], edges[:, 1])
    res = expLinkClassification(graph, HOPE(d=32, beta=0.01), rounds=3, ops=FEATURE_OPS + ('dot', 'method'), train_ratio=0.8, seed=0)
    print('operator     ROC-AUC   AP        (mean of 3 rounds)')
    for op, r in res.items():
        print('%-10s   %.4f    %.4f' % (op, np.mean(r['auc']), np.mean(r['ap'])))


if __name__ == '__main__':
    main()
