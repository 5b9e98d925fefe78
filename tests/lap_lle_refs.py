"""Graphs, fp64 references, float32 yardsticks and bars for Laplacian Eigenmaps and LLE on weighted, split and tiny graphs (tests/README_lap_lle.md).
Device-free: imported by test_lap_lle_refs.py (CPU) and test_lap_lle_edges_gpu.py.

Both methods are compared through the eigenvalues `lam` of the operator the solver iterates on and through invariant subspaces:
  lap   L = I - D^-1/2 A D^-1/2 (zero-degree nodes: D^-1/2 = 0, so they sit at eigenvalue 1),  lam = eigenvalue,        ||Op|| = 2
  lle   N = I - P, P = rows of A over their l1 norm (zero rows stay zero),                     lam = s^2 of N (N^T N),  ||Op|| = 1.05 sigma_max(N)^2
"""
import functools

import networkx as nx
import numpy as np

from gem_amd.graph import EdgeListGraph

TOL = 1e-6                # the solvers' default stopping tolerance: relative change of the wanted values
MARGIN = 4.0              # what this suite gives a float32 yardstick elsewhere (t-SNE, AP)
ORTHO_BAR = 5e-5          # test_lle_eigen_path_at_20k's bar on max |V^T V - I|
WIDE = 10.0               # a planted mistake must leave a bar by this factor


def f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------------------------ graphs
def planted(sizes, p_in, p_out, seed, loops=0):
    """Planted-partition nx.Graph on range(sum(sizes)) with float32 weights in [0.25, 4) and `loops` self-loops in [0.5, 2)."""
    rs = np.random.RandomState(seed)
    n = int(sum(sizes))
    block = np.repeat(np.arange(len(sizes)), sizes)
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for i in range(n):
        for j in range(i + 1, n):
            if rs.rand() < (p_in if block[i] == block[j] else p_out):
                G.add_edge(i, j, weight=f32(rs.uniform(.25, 4)))
    for v in rs.choice(n, loops, replace=False):
        G.add_edge(int(v), int(v), weight=f32(rs.uniform(.5, 2)))
    return G


def relabelled(G, n, position):
    """G's edges on range(n), node v of G at position[v]; the other positions stay zero-degree nodes."""
    H = nx.Graph()
    H.add_nodes_from(range(n))
    H.add_weighted_edges_from((int(position[a]), int(position[b]), wt) for a, b, wt in G.edges(data='weight'))
    return H


@functools.lru_cache(maxsize=None)
def weighted():
    return planted([60, 50, 50, 43], .25, .01, 7, loops=3)


ISOLATED_AT = (0, 101, 205)


@functools.lru_cache(maxsize=None)
def isolated():
    """`weighted` with three zero-degree nodes IN the node order (first, middle, last), not after it."""
    n = 206
    return relabelled(weighted(), n, np.setdiff1d(np.arange(n), ISOLATED_AT))


@functools.lru_cache(maxsize=None)
def isolated_appended():
    """The planted mistake: the same three nodes at the end."""
    return relabelled(weighted(), 206, np.arange(203))


@functools.lru_cache(maxsize=None)
def components():
    """Three components of two, two and one block, and one zero-degree node (the last)."""
    parts = [planted([40, 40], .3, .02, 11), planted([35, 25], .3, .02, 12), planted([20], .4, 0, 13)]
    H = nx.Graph()
    H.add_nodes_from(range(sum(len(p) for p in parts) + 1))
    off = 0
    for p in parts:
        H.add_weighted_edges_from((a + off, b + off, wt) for a, b, wt in p.edges(data='weight'))
        off += len(p)
    return H


def tiny():
    """test_edge_cases_gpu.tiny(): isolated node 4, self-loop on 2, sink 5, reciprocal arcs with different weights."""
    from test_edge_cases_gpu import tiny as edge_case_tiny
    return edge_case_tiny()


@functools.lru_cache(maxsize=None)
def asym_arcs():
    """(n, src, dst, w) of `weighted` as a directed multigraph listing: about 30 % of the edges as reciprocal arcs of two different weights, the rest
    as one arc of random orientation, five arcs listed a second time with another weight (a loop, two hi->lo and one lo->hi arc of reciprocal
    pairs, one single arc), all in shuffled order."""
    rs = np.random.RandomState(23)
    G = weighted()
    arcs, recip_down, recip_up, single, loop = [], [], [], [], []
    for a, b, wt in G.edges(data='weight'):
        lo, hi = min(a, b), max(a, b)
        if lo == hi:
            loop.append(len(arcs)); arcs.append((lo, lo, wt))
        elif rs.rand() < .3:
            recip_up.append(len(arcs)); arcs.append((lo, hi, wt))
            recip_down.append(len(arcs)); arcs.append((hi, lo, f32(rs.uniform(.25, 4))))
        else:
            single.append(len(arcs)); arcs.append((lo, hi, wt) if rs.rand() < .5 else (hi, lo, wt))
    again = [loop[0], recip_down[1], recip_down[4], recip_up[2], single[3]]
    arcs += [(arcs[e][0], arcs[e][1], f32(rs.uniform(.25, 4))) for e in again]
    order = rs.permutation(len(arcs))
    src, dst, w = (np.array([arcs[e][c] for e in order]) for c in range(3))
    return len(G), src.astype(np.int32), dst.astype(np.int32), w.astype(np.float32)


def asym(reverse=False):
    n, src, dst, w = asym_arcs()
    return EdgeListGraph(n, src[::-1], dst[::-1], w[::-1]) if reverse else EdgeListGraph(n, src, dst, w)


SIGNED_EDGES = 10


@functools.lru_cache(maxsize=None)
def signed():
    """`weighted` with ten non-loop edge weights negated (LLE only)."""
    G = weighted().copy()
    e = [(a, b) for a, b in G.edges() if a != b]
    for t in np.random.RandomState(29).choice(len(e), SIGNED_EDGES, replace=False):
        G.edges[e[t]]['weight'] = -G.edges[e[t]]['weight']
    return G


# name -> (graph, d values, cuts of the spectrum the subspaces are compared at for lap, for lle)
def case_graph(name):
    return {'weighted': weighted, 'isolated': isolated, 'components': components, 'tiny': lambda: tiny().to_networkx(), 'signed': signed}[name]()


CASE_D = {'weighted': (3,), 'isolated': (3,), 'components': (4,), 'tiny': (1, 2, 3, 4), 'signed': (3,)}
CASE_CUTS = {'weighted': (1, 4), 'isolated': (1, 4), 'components': (3, 5), 'tiny': (1, 2, 3, 4, 5), 'signed': (1, 4)}


# ------------------------------------------------------------------------------------------------------------------ fp64 references
def adjacency(G):
    """Dense fp64 adjacency of G.to_undirected() in G.nodes order, symmetrised by networkx (an EdgeListGraph goes through to_networkx())."""
    if isinstance(G, EdgeListGraph):
        G = G.to_networkx()
    return np.asarray(nx.to_scipy_sparse_array(G.to_undirected(), nodelist=list(G.nodes), dtype=np.float64, weight='weight').todense())


def adjacency_of_arrays(n, src, dst, w):
    """Dense fp64 matrix of what symmetric_arrays returns (both directions listed)."""
    A = np.zeros((n, n))
    A[np.asarray(src), np.asarray(dst)] = np.asarray(w, dtype=np.float64)
    return A


def lap_matrix(A, loop_twice=False, unweighted_degree=False):
    """L = I - D^-1/2 A D^-1/2 as lap_edge_values + (I + M) state it: a zero-degree node keeps its 1 on the diagonal.  The keyword arguments plant
    mistakes."""
    deg = (A != 0).sum(axis=1).astype(np.float64) if unweighted_degree else A.sum(axis=1)
    if loop_twice:
        deg = deg + np.diag(A)
    with np.errstate(divide='ignore'):
        dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    return np.eye(len(A)) - dinv[:, None] * A * dinv[None, :]


def lle_matrix(A, by_columns=False, use_abs=True):
    """N = I - P, P = A with rows over their l1 norm (sklearn normalize(norm='l1'): zero rows stay zero)."""
    l1 = (np.abs(A) if use_abs else A).sum(axis=1)
    inv = np.where(l1 != 0, 1.0 / np.where(l1 != 0, l1, 1.0), 0.0)
    return np.eye(len(A)) - (A * inv[None, :] if by_columns else inv[:, None] * A)


class Reference(object):
    """lam ascending (all n), U the matching vectors, norm = ||Op||, and the float32 yardstick of the same operator."""

    def __init__(self, kind, A):
        self.kind, self.n = kind, len(A)
        if kind == 'lap':
            self.lam, self.U = np.linalg.eigh(lap_matrix(A))
            self.norm = 2.0
            L32 = lap_matrix(A).astype(np.float32)                  # the device forms D^-1/2 A D^-1/2 in fp64 and rounds each entry once
            T32 = np.float32(2) * np.eye(self.n, dtype=np.float32) - L32
            mu, Z = np.linalg.eigvalsh(T32), np.linalg.eigh(T32)[1]
            assert mu.dtype == np.float32 and Z.dtype == np.float32
            self.lam32, self.U32 = (2.0 - mu.astype(np.float64))[::-1], Z[:, ::-1].astype(np.float64)
        else:
            N = lle_matrix(A)
            _, s, vt = np.linalg.svd(N)
            self.s, self.U = s[::-1], vt[::-1].T
            self.lam = self.s ** 2
            self.norm = 1.05 * s[0] ** 2
            c = np.float32(self.norm)
            N32 = N.astype(np.float32)                               # float32(w / l1) per entry, as lle_edge_values
            T32 = c * np.eye(self.n, dtype=np.float32) - N32.T @ N32
            mu, Z = np.linalg.eigvalsh(T32), np.linalg.eigh(T32)[1]
            assert mu.dtype == np.float32 and Z.dtype == np.float32
            self.lam32, self.U32 = (float(c) - mu.astype(np.float64))[::-1], Z[:, ::-1].astype(np.float64)

    def gap(self, j):
        return self.lam[j] - self.lam[j - 1]

    def angle(self, V, j):
        """||(I - U_j U_j^T) V[:, :j]||_2: the sine of the largest angle between span V[:, :j] and the reference's first j vectors when V is orthonormal."""
        Vj = np.asarray(V[:, :j], dtype=np.float64)
        Uj = self.U[:, :j]
        return float(np.linalg.norm(Vj - Uj @ (Uj.T @ Vj), 2))

    def value_bar(self, k):
        yard = float(np.abs(self.lam32[:k] - self.lam[:k]).max())
        return MARGIN * max(yard, TOL * self.norm), yard

    def subspace_bar(self, j):
        yard = self.angle(self.U32, j)
        return MARGIN * max(yard, np.sqrt(TOL * self.norm / self.gap(j))), yard

    def zero_rows_at(self, j):
        """The zero-degree nodes whose rows of U_j are zero (their own vector, at lam = 1, lies beyond the cut)."""
        return [i for i in self.zero_degree if np.abs(self.U[i, :j]).max() < 1e-12]


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    G = case_graph(name)
    A = adjacency(G)
    r = Reference(kind, A)
    r.zero_degree = [i for i in range(len(A)) if not np.abs(A[i]).any()]
    return r


def reference_of(kind, A):
    r = Reference(kind, A)
    r.zero_degree = [i for i in range(len(A)) if not np.abs(A[i]).any()]
    return r


# ------------------------------------------------------------------------------------------------------------------ checks
def measure(ref, V, lam_dev, cuts):
    """[(what, measured, bar)] for the device's V [n][k] and its k operator eigenvalues (lap: the eigenvalue; lle: s^2), ascending."""
    V = np.asarray(V, dtype=np.float64)
    lam_dev = np.asarray(lam_dev, dtype=np.float64)
    n, k = V.shape
    assert n == ref.n and lam_dev.shape == (k,)
    out = [('orthonormality max|V^T V - I|', float(np.abs(V.T @ V - np.eye(k)).max()), ORTHO_BAR)]
    bar, yard = ref.value_bar(k)
    out.append(('values max|lam - lam_ref| (float32 yardstick %.2e)' % yard, float(np.abs(lam_dev - ref.lam[:k]).max()), bar))
    for j in cuts:
        if j > k:
            continue
        bar, yard = ref.subspace_bar(j)
        out.append(('subspace at cut %d, gap %.4f (float32 yardstick %.2e)' % (j, ref.gap(j), yard), ref.angle(V, j), bar))
        rows = ref.zero_rows_at(j)
        if rows:
            out.append(('zero-degree rows %s at cut %d' % (rows, j), float(np.abs(V[rows, :j]).max()), bar))
    return out


def worst(measured):
    return max(m / bar for _, m, bar in measured)


def check(label, ref, V, lam_dev, cuts):
    """Prints every measured value against its bar, then asserts them all."""
    measured = measure(ref, V, lam_dev, cuts)
    for what, m, bar in measured:
        print('%s: %s: %.3e [bar %.3e]' % (label, what, m, bar))
    bad = [(what, m, bar) for what, m, bar in measured if not m <= bar]
    assert not bad, (label, bad)
    return measured


def span_distance(ref, Y, j):
    """Largest distance of a unit-normalised column of Y from the span of the reference's first j vectors."""
    Y = np.asarray(Y, dtype=np.float64)
    Y = Y / np.linalg.norm(Y, axis=0)
    Uj = ref.U[:, :j]
    return float(np.linalg.norm(Y - Uj @ (Uj.T @ Y), axis=0).max())


def first_listing_symmetric_arrays(g):
    """symmetric_arrays' EdgeListGraph rule before it followed networkx: the weight of a pair's FIRST listing in either direction.  The planted
    'other reciprocal-weight rule', and what undirected inputs must still give."""
    n = g.n
    s, d = g.src.astype(np.int64), g.dst.astype(np.int64)
    w = np.ones(len(s), np.float32) if g.w is None else g.w
    lo, hi = np.minimum(s, d), np.maximum(s, d)
    key, first = np.unique(lo * n + hi, return_index=True)
    lo, hi, w = key // n, key % n, w[first]
    loop = lo == hi
    src = np.concatenate([lo, hi[~loop]]); dst = np.concatenate([hi, lo[~loop]]); ww = np.concatenate([w, w[~loop]])
    return n, src.astype(np.int32), dst.astype(np.int32), ww.astype(np.float32)
