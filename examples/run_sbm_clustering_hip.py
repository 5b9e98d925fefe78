"""Community recovery on the SBM-1024 fixture graph on the GPU: embed with HOPE and with Laplacian Eigenmaps, cluster the rows with k-means
(k-means++ seeding, Lloyd) and score the clusters against the three planted blocks.  Laplacian Eigenmaps with unit-norm rows is spectral
clustering (Ng, Jordan, Weiss).  Five seeded rounds each.

    python examples/run_sbm_clustering_hip.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gem_amd.embedding.hope import HOPE                               # noqa: E402
from gem_amd.embedding.lap import LaplacianEigenmaps                  # noqa: E402
from gem_amd.evaluation.clustering import expClustering               # noqa: E402
from gem_amd.graph import EdgeListGraph                               # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def main():
    edges = np.load(os.path.join(GOLDEN, 'sbm1024_edges.npy'))
    labels = np.load(os.path.join(GOLDEN, 'sbm1024_labels.npy')).astype(np.int64)
    graph = EdgeListGraph(len(labels), edges[:, 0], edges[:, 1])
    runs = (('HOPE d=32', HOPE(d=32, beta=0.01), None), ('Laplacian Eigenmaps d=3, unit rows', LaplacianEigenmaps(d=3), 'l2'))
    print('embedding                               NMI      ARI      purity   (mean of 5 rounds)')
    for name, model, normalize in runs:
        X = np.asarray(model.learn_embedding(graph=graph), dtype=np.float32)
        res = expClustering(X, labels, rounds=5, seed=0, normalize=normalize)
        print('%-38s  %.4f   %.4f   %.4f' % (name, res['mean']['nmi'], res['mean']['ari'], res['mean']['purity']))


if __name__ == '__main__':
    main()
