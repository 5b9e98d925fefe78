"""The neighbourhood baselines of link prediction on the SBM-1024 fixture graph on the GPU -- the first rows of the node2vec paper's table 4:
hold out 20 % of the edges and rank the held-out edges against as many non-edges by common neighbours, Jaccard's coefficient, Adamic-Adar,
resource allocation and preferential attachment of the TRAIN graph.  No embedding is trained.  The second table puts two of them beside a
HOPE embedding's Hadamard classifier and inner product on the same pairs.  Three seeded rounds each.

    python examples/run_sbm_link_baselines_hip.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gem_amd.embedding.hope import HOPE                                          # noqa: E402
from gem_amd.evaluation.link_classification import expLinkClassification        # noqa: E402
from gem_amd.evaluation.link_heuristics import HEURISTICS, expLinkHeuristics     # noqa: E402
from gem_amd.graph import EdgeListGraph                                          # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def show(res):
    for name, r in res.items():
        print('%-10s   %.4f    %.4f' % (name, np.mean(r['auc']), np.mean(r['ap'])))


def main():
    edges = np.load(os.path.join(GOLDEN, 'sbm1024_edges.npy'))
    graph = EdgeListGraph(1024, edges[:, 0], edges[:, 1])
    print('score        ROC-AUC   AP        (mean of 3 rounds)')
    show(expLinkHeuristics(graph, rounds=3, which=HEURISTICS, train_ratio=0.8, seed=0))
    print('the same pairs, with an embedding (HOPE d = 32)')
    show(expLinkClassification(graph, HOPE(d=32, beta=0.01), rounds=3, ops=('hadamard', 'dot', 'cn', 'aa'), train_ratio=0.8, seed=0))


if __name__ == '__main__':
    main()
