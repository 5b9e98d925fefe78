"""Node classification of the SBM-1024 fixture graph on the GPU: embed with HOPE, then the one-vs-rest logistic fit and the top-k ranker
over test ratios 0.1 .. 0.9 (expNC, through GEM's import paths), five seeded rounds each.

    python examples/run_sbm_classification_hip.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gem.embedding.hope import HOPE                                   # noqa: E402
from gem.evaluation.evaluate_node_classification import expNC         # noqa: E402
from gem_amd.graph import EdgeListGraph                               # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def main():
    edges = np.load(os.path.join(GOLDEN, 'sbm1024_edges.npy'))
    labels = np.load(os.path.join(GOLDEN, 'sbm1024_labels.npy')).astype(np.int64)
    graph = EdgeListGraph(len(labels), edges[:, 0], edges[:, 1])
    X = np.asarray(HOPE(d=32, beta=0.01).learn_embedding(graph=graph), dtype=np.float64)
    X = (X - X.mean(axis=0)) / X.std(axis=0)          # the embedding's entries are ~1e-2: standardise, or the regulariser decides the fit
    ratios = [round(0.1 * r, 1) for r in range(1, 10)]
    res = expNC(X, labels, ratios, rounds=5, seed=0)
    print('test ratio   micro-F1   macro-F1   accuracy   (mean of 5 rounds)')
    for ratio in ratios:
        print('   %.1f       %.4f     %.4f     %.4f' % (ratio, np.mean(res[ratio]['micro']), np.mean(res[ratio]['macro']), np.mean(res[ratio]['accuracy'])))


if __name__ == '__main__':
    main()
