"""Link prediction: how well an embedding trained on the TRAIN part of a split ranks the held-out TEST edges.

The metric is a composition of functions of the reference, pinned by tests/golden/linkpred_ref.json (scripts/make_golden_linkpred.py runs them):
  gem/utils/evaluation_util.py:39-53   split_di_graph_to_train_test            -> gem_amd.utils.evaluation_util
  gem/utils/evaluation_util.py:28-35   get_edge_list_from_adj_mtrx (j != i, j > i when undirected, adj > 0)
  [e for e in edge_list if not train_digraph.has_edge(e[0], e[1])]            training edges leave the ranking
  gem/evaluation/metrics.py:6-46       computeMAP, computePrecisionCurve against the TEST graph

Candidates of node i: j != i, j > i when undirected, score(i, j) > 0, (i -> j) not a train arc; ordered by score descending, node id
ascending on ties (Python's stable sort of the ascending-j list).  Positives of i: its test neighbours that are candidates -- a test arc
that is also a train arc (the split leaves lone reverse arcs and self-loops in both graphs) is neither a hit nor a positive.
AP_i = mean over the positives of rank_hit / rank_all, 0 without a positive; MAP = sum AP_i / n (undirected) or over the nodes with test
out-degree > 0 (directed), as metrics.computeMAP counts.

Two tiers: dense numpy for small n (link_prediction_rows, link_prediction_dense), and the device evaluator of gem_amd/csrc/eval.hip
(evaluate_link_prediction_gpu: masked AP, per-node top-k, sampled pairs) for graphs whose n x n matrix cannot be formed.
"""
import numpy as np

from gem_amd.evaluation import reconstruction as gr

DENSE_MAX_N = 4096          # above this evaluateStaticLinkPrediction wants `nodes` or `sample_ratio_e`


def _without_train(score, train_truth):
    """The score matrix with every train arc at 0: `score > 0` then drops it from every candidate list."""
    s = np.array(score, dtype=np.float64)
    s[np.asarray(train_truth, dtype=bool)] = 0.0
    return s


def link_prediction_rows(score, train_truth, test_truth, undirected=True):
    """Per-node AP of link prediction from a dense score matrix: the CPU-tier counterpart of average_precision_rows.
    train_truth / test_truth: [n][n] bool, directed has_edge."""
    return gr.average_precision_rows(_without_train(score, train_truth), np.asarray(test_truth, dtype=bool), undirected=undirected)


def link_prediction_dense(score, train_truth, test_truth, is_undirected=True, max_k=None):
    """(MAP, prec_curv) exactly as computeMAP / computePrecisionCurve return them on the train-filtered edge list of
    get_edge_list_from_adj_mtrx(score); prec_curv is cut at max_k entries when given."""
    test_truth = np.asarray(test_truth, dtype=bool)
    s = _without_train(score, train_truth)
    n = s.shape[0]
    ap = gr.average_precision_rows(s, test_truth, undirected=is_undirected)
    if is_undirected:
        MAP = np.cumsum(ap)[-1] / n                                   # cumsum: Python's left-to-right sum(node_ap), metrics.py:46
    else:
        has_out = test_truth.any(axis=1)                              # metrics.py:37: nodes without a test successor do not count
        MAP = np.cumsum(ap[has_out])[-1] / int(has_out.sum()) if has_out.any() else 0.0
    prec = gr.precision_curve(s, test_truth, undirected=is_undirected, max_k=max_k)
    return float(MAP), prec.tolist()


def pairs_not_in_train(n, st, ed, train_src, train_dst):
    """keep[p] = not train.has_edge(st[p], ed[p]), by a lookup in the sorted keys src * n + dst of the train arcs."""
    key = np.unique(np.asarray(train_src, dtype=np.int64) * n + np.asarray(train_dst, dtype=np.int64))
    q = np.asarray(st, dtype=np.int64) * n + np.asarray(ed, dtype=np.int64)
    if key.size == 0:
        return np.ones(len(q), dtype=bool)
    pos = np.minimum(np.searchsorted(key, q), key.size - 1)
    return key[pos] != q


def evaluate_link_prediction_gpu(train_graph, test_graph, graph_embedding, X, nodes=None, sample_ratio_e=None, edge_pairs=None, k=None,
                                 is_undirected=True, seed=0):
    """Link prediction of the embedding X (trained on train_graph) against test_graph on the GPU, without an n x n matrix.  Both graphs are
    nx.DiGraph or EdgeListGraph over the same node ids.  One device handle holds the test graph; the train graph is its mask.
      * `sample_ratio_e` or `edge_pairs`: the pairs are scored and looked up in the test graph on the device (gemhip_eval_pairs), the pairs that
        are train arcs are dropped on the host, and pair_metrics returns (MAP, prec_curv) -- the reference's sample_ratio_e path.
      * otherwise `nodes`: returns a dict with 'nodes', 'ap' (per-node AP over ALL unmasked candidates, gemhip_eval_ap_masked), 'npos' (positives
        ranked per node) and 'MAP' (mean AP of the nodes computeMAP counts: all of `nodes` when undirected, those with a test successor otherwise).
        With `k` (1..1024) also 'topk_id', 'topk_score', 'topk_hit' ([len(nodes)][k]; id -1 pads a node with fewer candidates),
        'hits_at_k' (test arcs among a node's first k candidates) and 'precision_at_k' (= hits_at_k / k)."""
    from gem_amd.graph import edge_arrays
    n, tsrc, tdst, _, _ = edge_arrays(test_graph)
    n_train, rsrc, rdst, _, _ = edge_arrays(train_graph)
    if n_train != n:
        raise ValueError('evaluate_link_prediction_gpu: the train graph has %d nodes, the test graph %d' % (n_train, n))
    if edge_pairs is None and sample_ratio_e:
        edge_pairs = gr.random_edge_pairs(n, sample_ratio_e, is_undirected, seed)
    have_pairs = edge_pairs is not None and len(edge_pairs) > 0
    if not have_pairs and nodes is None:
        raise ValueError('evaluate_link_prediction_gpu: give sample_ratio_e, edge_pairs or nodes')
    with gr._DeviceEvaluator(n, tsrc, tdst, graph_embedding, X) as ev:
        if have_pairs:
            st, ed = gr._pair_arrays(edge_pairs)
            keep = pairs_not_in_train(n, st, ed, rsrc, rdst)
            st, ed = st[keep], ed[keep]
            score, hit = ev.pairs(st, ed)
            return gr.pair_metrics(n, st, ed, score, hit, is_undirected, out_degree=np.bincount(tsrc, minlength=n))
        nodes = np.ascontiguousarray(nodes, dtype=np.int64)
        ev.set_mask(rsrc, rdst)
        ap, npos = ev.ap_masked(nodes, is_undirected)
        counted = np.ones(len(nodes), dtype=bool) if is_undirected else np.bincount(tsrc, minlength=n)[nodes] > 0
        out = {'nodes': nodes, 'ap': ap, 'npos': npos, 'MAP': float(ap[counted].mean()) if counted.any() else 0.0}
        if k is not None:
            ids, score, hit = ev.topk(nodes, int(k), is_undirected, use_mask=True)
            out.update({'topk_id': ids, 'topk_score': score, 'topk_hit': hit, 'hits_at_k': hit.sum(axis=1).astype(np.int64)})
            out['precision_at_k'] = out['hits_at_k'] / float(k)
        return out


def restrict_to_train_lcc(train, test):
    """(train', test', new_of_old): the train graph cut down to its largest weakly connected component and renumbered (get_lcc), and the test
    graph restricted to the arcs between kept nodes, renumbered with the same map, in their original order."""
    from gem_amd.graph import EdgeListGraph
    from gem_amd.utils.graph_util import get_lcc
    train_lcc, new_of_old = get_lcc(train)
    s, d = new_of_old[test.src], new_of_old[test.dst]
    keep = (s >= 0) & (d >= 0)
    return train_lcc, EdgeListGraph(train_lcc.n, s[keep], d[keep], None if test.w is None else test.w[keep]), new_of_old


def evaluateStaticLinkPrediction(digraph, graph_embedding, train_ratio=0.8, nodes=None, sample_ratio_e=None, k=None, is_undirected=True, lcc=False):
    """Split `digraph` (split_di_graph_to_train_test: numpy's global stream, so np.random.seed reproduces the split), train
    `graph_embedding` on the train graph, evaluate against the test graph.  Returns (MAP, prec_curv).
    lcc=False (default): every node of `digraph` keeps its id -- X[i] is node i, and nodes the split isolates are embedded and ranked like any other.
    lcc=True: what upstream GEM's link-prediction driver does with graph_util.get_lcc after the split -- the train graph is replaced by its largest
    weakly connected component, renumbered 0..k-1 (gem_amd.utils.graph_util.get_lcc, on the GPU), the test graph is restricted to the kept nodes
    and renumbered with the same map, `nodes` (old ids) are mapped and the dropped ones left out; X then has one row per KEPT node and every
    figure below is over the renumbered pair.
      * neither `nodes` nor `sample_ratio_e`, n <= 4096: the dense host path (get_reconstructed_adj of the learned X, link_prediction_dense).
        Above that size one of the two is required.
      * `sample_ratio_e`: evaluate_link_prediction_gpu's pair path.
      * `nodes`: its per-node path; prec_curv is then None (`k` is passed through for its checks; call evaluate_link_prediction_gpu for the lists)."""
    from gem_amd.graph import edge_arrays
    from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
    train, test = split_di_graph_to_train_test(digraph, train_ratio, is_undirected)
    if lcc:
        train, test, new_of_old = restrict_to_train_lcc(train, test)
        if nodes is not None:
            nodes = new_of_old[np.asarray(nodes, dtype=np.int64)]
            nodes = nodes[nodes >= 0]
    n = test.n
    if nodes is None and not sample_ratio_e and n > DENSE_MAX_N:
        raise ValueError('evaluateStaticLinkPrediction: %d nodes is above the dense limit of %d: give `nodes` (per-node AP on the GPU) or '
                         '`sample_ratio_e` (sampled pairs)' % (n, DENSE_MAX_N))
    X = graph_embedding.learn_embedding(graph=train, no_python=True)
    if isinstance(X, tuple):                                          # (X, seconds) of older plug-ins
        X = X[0]
    if nodes is None and not sample_ratio_e:
        train_truth = gr._adjacency_bool(train, n); test_truth = gr._adjacency_bool(test, n)
        return link_prediction_dense(graph_embedding.get_reconstructed_adj(X), train_truth, test_truth, is_undirected)
    if sample_ratio_e:
        return evaluate_link_prediction_gpu(train, test, graph_embedding, X, sample_ratio_e=sample_ratio_e, is_undirected=is_undirected)
    res = evaluate_link_prediction_gpu(train, test, graph_embedding, X, nodes=nodes, k=k, is_undirected=is_undirected)
    return res['MAP'], None
