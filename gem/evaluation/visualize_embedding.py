"""Minimal 2-D scatter of an embedding for GEM-style drivers (plotting is out of scope of the backend, SURVEY section 2 #13;
this keeps `from gem.evaluation import visualize_embedding as viz` importable).  d > 2 is projected on its first two
principal components by default (upstream uses t-SNE); reduce='tsne' is upstream's t-SNE, on the GPU."""
import numpy as np


def reduce_to_2d(node_pos, reduce='pca'):
    """The points plot_embedding2D draws.  d <= 2: as they are.  d > 2:
    reduce='pca'  (default) the first two principal components, on the host;
    reduce='tsne' gem_amd.evaluation.tsne.tsne_2d with its defaults (perplexity 30, PCA init, 1000 iterations): needs the GPU."""
    if reduce not in ('pca', 'tsne'):
        raise ValueError("reduce must be 'pca' or 'tsne'")
    X = np.asarray(node_pos, dtype=float)
    if X.shape[1] > 2:
        if reduce == 'tsne':
            from gem_amd.evaluation.tsne import tsne_2d
            return tsne_2d(X)[0]
        Xc = X - X.mean(axis=0)
        _, _, vt = np.linalg.svd(Xc, full_matrices=False)
        X = Xc @ vt[:2].T
    return X


def plot_embedding2D(node_pos, node_colors=None, di_graph=None, labels=None, reduce='pca'):
    """reduce: how d > 2 becomes two dimensions, 'pca' (default) or 'tsne' (see reduce_to_2d)."""
    import matplotlib.pyplot as plt
    X = reduce_to_2d(node_pos, reduce)
    if di_graph is not None:
        for i, j in di_graph.edges():
            plt.plot([X[i, 0], X[j, 0]], [X[i, 1], X[j, 1]], color='0.8', linewidth=0.5, zorder=1)
    plt.scatter(X[:, 0], X[:, 1], c=node_colors, s=25, zorder=2)
