"""Restatements for the neighbourhood link-prediction scores (gem_amd/csrc/nbr.hip) in numpy / scipy: the simple undirected CSR of an arc
list, the degrees, the five scores through the row product A[st].multiply(A[ed]), the correctly rounded sum (math.fsum) of a given weight
table over each intersection, the planner's counts in three lines -- and the graphs the tests are built on."""
import math

import numpy as np
import scipy.sparse as sp

LANES, NARROW, CHUNK = 16, 32, 2048          # gemhip_nbr_info[3:6]: the shapes of the tests straddle them
HEURISTICS = ('cn', 'jaccard', 'aa', 'ra', 'pa')


def simple_csr(n, src, dst):
    """scipy CSR, 0 / 1 int64: both orientations merged, self-loops dropped, repeats merged; sorted indices."""
    src = np.asarray(src, dtype=np.int64); dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    s = np.concatenate([src[keep], dst[keep]]); d = np.concatenate([dst[keep], src[keep]])
    A = sp.csr_matrix((np.ones(len(s), np.int64), (s, d)), shape=(n, n))
    A.sum_duplicates()
    A.data[:] = 1
    A.sort_indices()
    return A


def degrees(A):
    return np.diff(A.indptr).astype(np.int32)


def weight_tables(deg):
    """(w_aa, w_ra) float64: 1 / ln(deg) where deg >= 2 and 1 / deg where deg >= 1, 0 elsewhere; ln is the machine's libm (math.log)."""
    deg = np.asarray(deg)
    w_aa = np.array([1.0 / math.log(float(k)) if k >= 2 else 0.0 for k in deg.tolist()])
    w_ra = np.array([1.0 / float(k) if k >= 1 else 0.0 for k in deg.tolist()])
    return w_aa, w_ra


def scores(A, st, ed, w_aa=None, w_ra=None):
    """{'cn' int32, 'jaccard', 'aa', 'ra', 'pa' float64} of the pairs: I = A[st].multiply(A[ed]), its row sums plain and weighted."""
    st = np.asarray(st); ed = np.asarray(ed)
    deg = degrees(A)
    if w_aa is None:
        w_aa, w_ra = weight_tables(deg)
    I = A[st].multiply(A[ed]).tocsr()
    cn = np.asarray(I.sum(1)).ravel().astype(np.int64)
    du, dv = deg[st].astype(np.int64), deg[ed].astype(np.int64)
    union = du + dv - cn
    jac = np.zeros(len(st))
    np.divide(cn.astype(np.float64), union.astype(np.float64), out=jac, where=union > 0)
    return {'cn': cn.astype(np.int32), 'jaccard': jac, 'aa': np.asarray(I @ w_aa).ravel(), 'ra': np.asarray(I @ w_ra).ravel(),
            'pa': du.astype(np.float64) * dv.astype(np.float64)}


def fsum_scores(table, A, st, ed):
    """float64 (m,): math.fsum of table[w] over w in the intersection of the two rows, per pair -- the correctly rounded sum."""
    table = np.asarray(table, dtype=np.float64)
    out = np.zeros(len(st))
    ip, ix = A.indptr, A.indices
    for p, (u, v) in enumerate(zip(np.asarray(st).tolist(), np.asarray(ed).tolist())):
        both = np.intersect1d(ix[ip[u]:ip[u + 1]], ix[ip[v]:ip[v + 1]], assume_unique=True)
        out[p] = math.fsum(table[both].tolist())
    return out


def sum_bound(cn, ref):
    """(k + 1) 2^-53 ref: k - 1 additions in any order of positive terms, and fsum's own rounding."""
    return (np.asarray(cn, dtype=np.float64) + 1.0) * 2.0 ** -53 * np.asarray(ref)


def plan_counts(deg, st, ed):
    """(narrow items, wide items, split pairs, partial slots) of the planner, restated."""
    la = np.minimum(np.asarray(deg)[np.asarray(st)], np.asarray(deg)[np.asarray(ed)]).tolist()
    lens = [min(CHUNK, l - s) for l in la for s in range(0, l, CHUNK)]
    return sum(x <= NARROW for x in lens), sum(x > NARROW for x in lens), sum(l > CHUNK for l in la), sum(-(-l // CHUNK) for l in la if l > CHUNK)


# ------------------------------------------------------------------ graphs
def two_hub_graph(la, lb, overlap):
    """(n, src, dst, A, B): hubs A = 0 and B = 1 with la and lb neighbours, `overlap` of them shared.  Shared node i is also tied to i % 8
    of eight filler nodes, so the shared nodes have degrees 2 .. 9 and their weights differ; every other neighbour is a leaf."""
    assert 0 <= overlap <= la <= lb
    fill = np.arange(2, 10)
    shared = 10 + np.arange(overlap)
    only_a = 10 + overlap + np.arange(la - overlap)
    only_b = 10 + la + np.arange(lb - overlap)
    n = 10 + la + lb - overlap
    src = [np.zeros(la, np.int64), np.ones(lb, np.int64)]
    dst = [np.concatenate([shared, only_a]), np.concatenate([shared, only_b])]
    for i, w in enumerate(shared.tolist()):
        k = i % 8
        src.append(np.full(k, w)); dst.append(fill[:k])
    src = np.concatenate(src); dst = np.concatenate(dst)
    flip = np.arange(len(src)) % 2 == 1                       # one-sided arcs in either direction
    s = np.where(flip, dst, src).astype(np.int32); d = np.where(flip, src, dst).astype(np.int32)
    return int(n), s, d, 0, 1


def hand_graph():
    """12 nodes: a triangle 0-1-2, a tail 2-3-4, a star 5-(6,7,8), 9-10 apart, 11 isolated; with a self-loop, a repeat and both orientations."""
    e = [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (5, 6), (5, 7), (5, 8), (9, 10), (1, 0), (0, 1), (3, 3), (6, 1), (7, 1)]
    return 12, np.array([a for a, _ in e], np.int32), np.array([b for _, b in e], np.int32)
