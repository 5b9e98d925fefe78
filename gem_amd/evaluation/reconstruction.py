"""Graph-reconstruction metric (MAP, precision curve) -- vectorised restatement of
GEM's evaluator, used as THE parity metric of this backend.

Mirrors, result-for-result (pinned by tests/golden/map_ref.json, which was
produced by the reference's own code):
  gem/evaluation/evaluate_graph_reconstruction.py:8-46   evaluateStaticGraphReconstruction
  gem/utils/evaluation_util.py:20-36                     get_edge_list_from_adj_mtrx (i<j, adj>0)
  gem/evaluation/metrics.py:6-24, 27-46                  computePrecisionCurve, computeMAP

The reference builds Python lists of (i, j, w) tuples and sorts them (O(n^2) Python
objects); here every node's candidate list is one stable argsort over a numpy
row, so n ~ 2e4 is practical.  Tie order follows the reference: Python's stable
`sorted(..., reverse=True)` keeps equal weights in ascending-j order.

Pair-sampled evaluation (the reference's `sample_ratio_e`, its own answer to large graphs):
  gem/utils/evaluation_util.py:5-17    get_random_edge_pairs        -> random_edge_pairs
  gem/utils/evaluation_util.py:23-26   edge list of the sampled pairs (adj >= 0)  \
  gem/evaluation/metrics.py:6-46       precision curve and MAP over that list     -> pair_metrics
pinned by tests/golden/eval_pairs_ref.json (scripts/make_golden_eval_pairs.py runs the reference's functions).
evaluate_reconstruction_gpu returns the reference's whole tuple (MAP, prec_curv, err, err_baseline) from the device
(gem_amd/csrc/eval.hip) without an n x n matrix, for all five methods.
"""
import numpy as np

from gem_amd.evaluation._handle import DeviceHandle


def _adjacency_bool(digraph, n):
    A = np.zeros((n, n), dtype=bool)
    if hasattr(digraph, 'src'):
        A[digraph.src, digraph.dst] = True
    else:
        for i, j in digraph.edges():
            A[i, j] = True
    return A


def average_precision_rows(score, truth, undirected=True):
    """Per-node AP exactly as metrics.computeMAP: node i ranks candidates j (j>i when
    undirected) with score>0 by descending score; AP_i = mean precision at the hits."""
    n = score.shape[0]
    ap = np.zeros(n)
    for i in range(n):
        lo = i + 1 if undirected else 0
        s = score[i, lo:]
        t = truth[i, lo:]
        if not undirected:
            keep = np.ones(s.shape[0], dtype=bool)
            keep[i] = False
            s, t = s[keep], t[keep]
        pos = s > 0
        s, t = s[pos], t[pos]
        if s.size == 0:
            continue
        order = np.argsort(-s, kind='stable')
        hit = t[order]
        nh = hit.sum()
        if nh == 0:
            continue
        prec = np.cumsum(hit) / np.arange(1, hit.size + 1)
        ap[i] = prec[hit].sum() / nh
    return ap


def precision_curve(score, truth, undirected=True, max_k=None):
    n = score.shape[0]
    iu = np.triu_indices(n, 1) if undirected else np.where(~np.eye(n, dtype=bool))
    s = score[iu]
    t = truth[iu]
    pos = s > 0
    s, t = s[pos], t[pos]
    order = np.argsort(-s, kind='stable')
    hit = t[order]
    if max_k is not None:
        hit = hit[:max_k]
    return np.cumsum(hit) / np.arange(1, hit.size + 1)


def evaluateStaticGraphReconstruction(digraph, graph_embedding, X_stat, node_l=None, file_suffix=None,
                                      sample_ratio_e=None, is_undirected=True, is_weighted=False, edge_pairs=None, seed=0):
    """Same signature and return tuple as the reference: (MAP, prec_curv, err, err_baseline).
    With `sample_ratio_e` (or an explicit `edge_pairs` list of (st, ed)) only those node pairs are scored, as the reference does
    (evaluate_graph_reconstruction.py:14-19); the sample is random_edge_pairs(n, sample_ratio_e, is_undirected, seed)."""
    n = len(digraph.nodes)
    est = graph_embedding.get_reconstructed_adj(X_stat, node_l)
    truth = _adjacency_bool(digraph, n)
    if edge_pairs is None and sample_ratio_e:
        edge_pairs = random_edge_pairs(n, sample_ratio_e, is_undirected, seed)
    if edge_pairs is not None and len(edge_pairs):                   # evaluation_util.py:23: an empty list means "all pairs"
        st, ed = _pair_arrays(edge_pairs)
        MAP, prec = pair_metrics(n, st, ed, est[st, ed], truth[st, ed], is_undirected, out_degree=truth.sum(axis=1))
        prec = np.asarray(prec)
    else:
        ap = average_precision_rows(est, truth, undirected=is_undirected)
        if is_undirected:
            MAP = ap.sum() / n
        else:
            has_out = truth.any(axis=1)
            MAP = ap[has_out].sum() / max(int(has_out.sum()), 1)
        prec = precision_curve(est, truth, undirected=is_undirected)
    err = err_base = None
    if is_weighted:
        W = np.zeros((n, n))
        for i, j, w in digraph.edges(data='weight', default=1):
            W[i, j] = w
        e = est.copy()
        e[W == 0] = 0
        err = np.linalg.norm(W - e)
        err_base = np.linalg.norm(W)
    return float(MAP), prec.tolist(), err, err_base


def _pair_arrays(edge_pairs):
    p = np.asarray(edge_pairs, dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1])


def random_edge_pairs(n, sample_ratio, is_undirected=True, seed=0):
    """Seeded, vectorised restatement of get_random_edge_pairs (evaluation_util.py:5-17): distinct ordered pairs (st, ed) drawn
    uniformly from [0, n)^2; in undirected mode no pair appears together with its reverse; self-pairs are allowed, as in the reference.
    The count is the reference loop's: int(r n (n-1)) directed, ceil(int(r n (n-1)) / 2) undirected (it compares len(set) < num_pairs / 2
    as a float).  The reference draws from `secrets` and returns list(set), so its sample cannot be reproduced; this one is a function
    of `seed`.  Returns an int64 array [count, 2] in draw order -- that order is the tie order of everything downstream (pair_metrics
    sorts stably, as metrics.py sorts the reference's list)."""
    n = int(n)
    count = int(sample_ratio * n * (n - 1))
    if is_undirected:
        count = (count + 1) // 2
    limit = n * (n + 1) // 2 if is_undirected else n * n
    if count > limit:
        raise ValueError('random_edge_pairs: %d pairs asked of %d nodes, only %d exist' % (count, n, limit))
    rng = np.random.default_rng(seed)
    a = np.empty(0, dtype=np.int64); b = np.empty(0, dtype=np.int64)
    while len(a) < count:
        m = int(1.1 * (count - len(a))) + 64
        a = np.concatenate([a, rng.integers(0, n, size=m, dtype=np.int64)])
        b = np.concatenate([b, rng.integers(0, n, size=m, dtype=np.int64)])
        key = np.minimum(a, b) * n + np.maximum(a, b) if is_undirected else a * n + b
        first = np.sort(np.unique(key, return_index=True)[1])          # first appearance of every pair, in draw order
        a, b = a[first], b[first]
    return np.stack([a[:count], b[:count]], axis=1)


def _left_to_right_group_sums(v, start, size, small=32):
    """Sum of every group v[start[g] : start[g] + size[g]] added left to right, as Python's sum() in metrics.py:45 does -- numpy's own
    reductions add pairwise, which moves the last bit.  Groups of up to `small` elements advance together, one position per step;
    the few longer ones go through cumsum one by one."""
    out = np.zeros(len(start))
    short = np.flatnonzero(size <= small)
    if len(short):
        short = short[np.argsort(-size[short], kind='stable')]        # longest first: step k touches a prefix
        sz = size[short]
        for k in range(int(sz[0])):
            live = short[:np.searchsorted(-sz, -k, side='left')]      # groups with size > k
            out[live] += v[start[live] + k]
    for gidx in np.flatnonzero(size > small):
        out[gidx] = np.cumsum(v[start[gidx]:start[gidx] + size[gidx]])[-1]
    return out


def pair_metrics(n, st, ed, score, hit, is_undirected=True, out_degree=None):
    """(MAP, prec_curv) of a scored pair list, exactly as the reference computes them from get_edge_list_from_adj_mtrx(edge_pairs=...):
    pairs with score >= 0 are kept (evaluation_util.py:25 -- `>=`, not the `>` of the all-pairs path at :34); the precision curve is the
    cumulative hit rate over all kept pairs in stable descending score order (metrics.py:6-24); MAP groups the pairs by `st`, sorts each
    group the same way, AP = mean precision at the hits (0 without hits), summed over nodes and divided by n (undirected) or by the
    number of nodes with out-degree > 0, whose APs alone count (directed; metrics.py:27-46).  `hit[p]` says whether st[p] -> ed[p] is an
    edge; `out_degree` (length n) is needed in directed mode.  Ties keep the order of the list."""
    st = np.asarray(st, dtype=np.int64); score = np.asarray(score, dtype=np.float64); hit = np.asarray(hit).astype(bool)
    keep = score >= 0.0
    st, score, hit = st[keep], score[keep], hit[keep]
    m = len(score)
    order = np.argsort(-score, kind='stable')
    prec_curv = (np.cumsum(hit[order]) / np.arange(1, m + 1)).tolist()
    ap = np.zeros(n)
    if m:
        order = np.lexsort((-score, st))                              # by st, then stable descending score
        g = st[order]; h = hit[order].astype(np.float64)
        start = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
        first = np.repeat(start, np.diff(np.r_[start, m]))            # index of each pair's group start
        cum = np.cumsum(h)
        before = (cum - h)[first]
        prec = (cum - before) / (np.arange(m) - first + 1)
        nodes = g[start]
        nh = np.add.reduceat(h, start)                                # (integers: exact in any order)
        sums = _left_to_right_group_sums(prec * h, start, np.diff(np.r_[start, m]))
        ap[nodes] = np.where(nh > 0, sums / np.maximum(nh, 1), 0.0)
    if is_undirected:
        return float(np.cumsum(ap)[-1] / n), prec_curv               # cumsum: Python's left-to-right sum(node_ap), metrics.py:46
    if out_degree is None:
        raise ValueError('pair_metrics: directed MAP needs out_degree (metrics.py:37 skips nodes without successors)')
    has_out = np.asarray(out_degree) > 0
    ap[~has_out] = 0.0
    return float(np.cumsum(ap)[-1] / max(int(has_out.sum()), 1)), prec_curv


def sampled_map(graph, pair_score, nodes, undirected=True):
    """MAP over a sample of nodes for graphs where the n x n matrix cannot be formed
    (SURVEY 8f row 1).  `pair_score(i) -> scores of node i against all nodes` (length n).
    Equals computeMAP restricted to `nodes` (tested against the full evaluator)."""
    n = graph.number_of_nodes()
    if hasattr(graph, 'src'):
        order = np.argsort(graph.src, kind='stable')
        s_sorted = graph.src[order]
        d_sorted = graph.dst[order]
        starts = np.searchsorted(s_sorted, np.arange(n + 1))
        nbrs = lambda i: d_sorted[starts[i]:starts[i + 1]]
    else:
        nbrs = lambda i: np.fromiter(graph.successors(i), dtype=np.int64)
    aps = []
    for i in nodes:
        s = np.asarray(pair_score(i), dtype=np.float64).copy()
        t = np.zeros(n, dtype=bool)
        t[nbrs(i)] = True
        lo = i + 1 if undirected else 0
        s, t = s[lo:], t[lo:]
        if not undirected:
            s[i] = 0
        pos = s > 0
        s, t = s[pos], t[pos]
        if s.size == 0 or t.sum() == 0:
            aps.append(0.0)
            continue
        hit = t[np.argsort(-s, kind='stable')]
        prec = np.cumsum(hit) / np.arange(1, hit.size + 1)
        aps.append(prec[hit].sum() / hit.sum())
    return float(np.mean(aps)) if aps else 0.0


def eligible_sample(graph, size, seed=1):
    """A node sample for sampled MAP on graphs where a uniform sample is mostly dead weight.  metrics.computeMAP ranks, for node i, the candidates j > i
    only (evaluation_util.py:28-35 lists the upper triangle): a node without a neighbour j > i has AP 0 whatever the embedding.  On a power-law graph that is
    two thirds of the nodes, the remaining APs are small and heavy-tailed, and a 2048-node uniform sample of R-MAT scale 17 sums to ~11: ONE node whose only
    neighbour lands on rank 1 moves the "MAP" by 9 %.  This draws `size` nodes (sorted; RandomState(seed), without replacement) from the nodes that have
    such a neighbour -- every sampled node carries information, and paired launch-to-launch comparisons get a standard error of ~0.3 % at 16 384 nodes."""
    from gem_amd.graph import edge_arrays
    n, src, dst, _, _ = edge_arrays(graph)
    elig = np.unique(src[dst > src])
    return np.sort(np.random.RandomState(seed).choice(elig, size=min(int(size), len(elig)), replace=False)).astype(np.int64)


def _score_operands(graph_embedding, X):
    """(A, B, kind) of the device score for a method's get_edge_weight."""
    X = np.asarray(X)
    name = graph_embedding.get_method_name() if graph_embedding is not None else ''
    if name == 'hope_gsvd':                                   # hope.py:43-44: X[i, :k] . X[j, k:]
        k = X.shape[1] // 2
        return np.ascontiguousarray(X[:, :k], dtype=np.float32), np.ascontiguousarray(X[:, k:2 * k], dtype=np.float32), 0
    if name in ('', 'graph_factor_sgd', 'node2vec_rw'):       # gf.py:103-104 / node2vec.py:56-57: X[i] . X[j]
        return np.ascontiguousarray(X, dtype=np.float32), None, 0
    if name in ('lap_eigmap_svd', 'lle_svd'):                 # lap.py:74 / lle.py:53: exp(-||x_i - x_j||^2)
        return np.ascontiguousarray(X, dtype=np.float32), None, 1
    raise NotImplementedError('no device score for %r: its get_edge_weight is neither an inner product nor exp(-||x_i - x_j||^2) '
                              '-- use evaluateStaticGraphReconstruction' % name)


class _DeviceEvaluator(DeviceHandle):
    """gemhip_eval_* handle: embedding and CSR (columns sorted) of the true graph on the device, uploaded once."""

    _destroy = 'gemhip_eval_destroy'

    def __init__(self, n, src, dst, graph_embedding, X):
        import ctypes as C
        from gem_amd import _hip
        from gem_amd.graph import to_csr
        self._hip, self._C = _hip, C
        A, B, kind = _score_operands(graph_embedding, X)
        if A.shape[0] != n:
            raise ValueError('embedding has %d rows, the graph %d nodes' % (A.shape[0], n))
        row_ptr, col, _ = to_csr(n, src, dst, None, sort_cols=True)
        DeviceHandle.__init__(self)
        self.n = n
        _hip.check(_hip.lib().gemhip_eval_create(n, A.shape[1], A.shape[1], _hip.ptr(A, C.c_float), _hip.ptr(B, C.c_float), kind,
                                                 _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), C.byref(self._h)))

    def ap(self, nodes, is_undirected):
        C, _hip = self._C, self._hip
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        out = np.zeros(len(nodes))
        _hip.check(_hip.lib().gemhip_eval_ap(self._h, 1 if is_undirected else 0, len(nodes), _hip.ptr(nodes, C.c_int32), _hip.ptr(out, C.c_double)))
        return out

    def pairs(self, st, ed, want_hit=True):
        C, _hip = self._C, self._hip
        st = np.ascontiguousarray(st, dtype=np.int32); ed = np.ascontiguousarray(ed, dtype=np.int32)
        score = np.zeros(len(st)); hit = np.zeros(len(st), dtype=np.uint8) if want_hit else None
        _hip.check(_hip.lib().gemhip_eval_pairs(self._h, len(st), _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(score, C.c_double),
                                                _hip.ptr(hit, C.c_uint8)))
        return score, hit

    def set_mask(self, src=None, dst=None):
        """The train graph of link prediction (gem_amd/evaluation/link_prediction.py): arcs (src -> dst) leave every candidate list of
        ap_masked and topk.  set_mask() without arguments clears it."""
        C, _hip = self._C, self._hip
        if src is None:
            _hip.check(_hip.lib().gemhip_eval_set_mask(self._h, None, None))
            return
        from gem_amd.graph import to_csr
        row_ptr, col, _ = to_csr(self.n, src, dst, None)
        _hip.check(_hip.lib().gemhip_eval_set_mask(self._h, _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32)))

    def ap_masked(self, nodes, is_undirected):
        """(AP, number of ranked positives) per node, train arcs masked out."""
        C, _hip = self._C, self._hip
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        out = np.zeros(len(nodes)); npos = np.zeros(len(nodes), dtype=np.int64)
        _hip.check(_hip.lib().gemhip_eval_ap_masked(self._h, 1 if is_undirected else 0, len(nodes), _hip.ptr(nodes, C.c_int32), _hip.ptr(out, C.c_double),
                                                    _hip.ptr(npos, C.c_int64)))
        return out, npos

    def topk(self, nodes, k, is_undirected, use_mask=True):
        """(id, score, hit), each [len(nodes)][k]: every node's k best candidates in the evaluator's order; id -1 pads a short list."""
        C, _hip = self._C, self._hip
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        ids = np.zeros((len(nodes), k), dtype=np.int32); score = np.zeros((len(nodes), k)); hit = np.zeros((len(nodes), k), dtype=np.uint8)
        _hip.check(_hip.lib().gemhip_eval_topk(self._h, 1 if is_undirected else 0, 1 if use_mask else 0, len(nodes), _hip.ptr(nodes, C.c_int32), int(k),
                                               _hip.ptr(ids, C.c_int32), _hip.ptr(score, C.c_double), _hip.ptr(hit, C.c_uint8)))
        return ids, score, hit

    def last_kernel_ms(self):
        ms = self._C.c_double(0.0)
        self._hip.check(self._hip.lib().gemhip_eval_last_kernel_ms(self._h, self._C.byref(ms)))
        return ms.value

    def last_pairs_ms(self):
        ms = self._C.c_double(0.0)
        self._hip.check(self._hip.lib().gemhip_eval_last_pairs_ms(self._h, self._C.byref(ms)))
        return ms.value


def sampled_ap_gpu(graph, graph_embedding, X, nodes, is_undirected=True):
    """Per-node AP of graph reconstruction for `nodes`, computed on the GPU (gem_amd/csrc/eval.hip) with the same
    semantics as average_precision_rows / metrics.computeMAP -- no n x n matrix, so it works at 1M nodes.
    mean() of the result over ALL nodes equals evaluateStaticGraphReconstruction's MAP (tests/test_eval_gpu.py).
    GF, node2vec and HOPE score by inner products; Laplacian Eigenmaps and LLE by the scalar get_edge_weight
    exp(-norm(x_i - x_j)^2) in fp64 (not the expanded sq_i + sq_j - 2 x.y form, which cancels).  Ranks and ties are decided on
    the exp output: where exp saturates (eigenvectors of a 1M-node graph differ by ~1e-6) distinct distances share one tie class,
    broken by node id as in the reference; there the tie classes are those of the device's fp64 exp, which may differ from
    glibc's by one ulp."""
    from gem_amd.graph import edge_arrays
    n, src, dst, w, _ = edge_arrays(graph)
    with _DeviceEvaluator(n, src, dst, graph_embedding, X) as ev:
        return ev.ap(nodes, is_undirected)


def evaluate_reconstruction_gpu(graph, graph_embedding, X, sample_ratio_e=None, edge_pairs=None, nodes=None, is_undirected=True,
                                is_weighted=False, seed=0):
    """The reference evaluator's return tuple (MAP, prec_curv, err, err_baseline) computed on the GPU without an n x n matrix, for
    GF, node2vec, HOPE, Laplacian Eigenmaps and LLE, on an nx.DiGraph or an EdgeListGraph.  One device handle serves all parts.
      * `sample_ratio_e` or `edge_pairs` ([m, 2] or a list of (st, ed)): the pairs are scored on the device and MAP / prec_curv come from
        pair_metrics -- the reference's sample_ratio_e path; the sample is random_edge_pairs(n, sample_ratio_e, is_undirected, seed).
      * otherwise `nodes`: MAP = mean AP of those nodes over ALL their candidates (sampled_ap_gpu), prec_curv is None.
      * `is_weighted`: err = sqrt(sum over edges (w_ij - s_ij)^2) with s from the device, a self-loop contributing w^2 (the
        reconstructed diagonal is zero) and a zero-weight edge nothing; err_baseline = ||w||_2: evaluate_graph_reconstruction.py:38-42
        without the dense matrices.  The edge list must not hold the same (i, j) twice (a dense adjacency would hold it once).
    Scores are those of the fp32-rounded embedding, accumulated in fp64 (see sampled_ap_gpu for the exp of LE / LLE)."""
    from gem_amd.graph import edge_arrays
    n, src, dst, w, _ = edge_arrays(graph)
    if edge_pairs is None and sample_ratio_e:
        edge_pairs = random_edge_pairs(n, sample_ratio_e, is_undirected, seed)
    have_pairs = edge_pairs is not None and len(edge_pairs) > 0
    if not have_pairs and nodes is None and not is_weighted:
        raise ValueError('evaluate_reconstruction_gpu: give sample_ratio_e, edge_pairs or nodes (or is_weighted for the edge error alone)')
    MAP = prec = err = err_base = None
    with _DeviceEvaluator(n, src, dst, graph_embedding, X) as ev:
        if have_pairs:
            st, ed = _pair_arrays(edge_pairs)
            score, hit = ev.pairs(st, ed)
            MAP, prec = pair_metrics(n, st, ed, score, hit, is_undirected, out_degree=np.bincount(src, minlength=n))
        elif nodes is not None:
            ap = ev.ap(nodes, is_undirected)
            MAP = float(ap.mean()) if len(ap) else 0.0
        if is_weighted:
            ww = np.ones(len(src)) if w is None else np.asarray(w, dtype=np.float64)
            s, _ = ev.pairs(src, dst, want_hit=False)
            s[ww == 0] = 0.0                                           # estimated_adj[digraph_adj == 0] = 0
            err = float(np.sqrt(np.sum((ww - s) ** 2)))
            err_base = float(np.sqrt(np.sum(ww ** 2)))
    return MAP, prec, err, err_base
