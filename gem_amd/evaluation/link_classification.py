"""Link prediction as classification on the GPU (gem_amd/csrc/edgeclf.hip, rank.hip): the protocol of the node2vec paper
(section 4.4, table 4) and most of the link-prediction literature.  Held-out edges and as many non-edges are the test pairs; a pair becomes a
feature vector through a binary operator on its two embedding rows (average, Hadamard, weighted-L1, weighted-L2); a logistic regression is
fitted on the training pairs -- the exact minimiser of sklearn's LogisticRegression(C) objective, by the node-classification solver -- and
the test pairs are ranked by their logit: ROC-AUC and average precision.  op='dot' ranks by the plain inner product without a fit,
op='method' by the embedding method's own edge weight (the only direction-aware choice: HOPE on directed graphs).
Sampling is host code; everything else runs on the device.  No host fallback: GemHipError without a device."""
import ctypes as ct
import time
import warnings

import numpy as np

from gem_amd import _hip
from gem_amd.evaluation._handle import DeviceHandle, embedding_matrix
from gem_amd.evaluation import ranking
from gem_amd.evaluation.link_heuristics import HEURISTICS, NeighbourScorer
from gem_amd.evaluation.node_classification import DEC_TOL, MAX_ITER

OPERATORS = {'average': 0, 'hadamard': 1, 'l1': 2, 'l2': 3}
FEATURE_OPS = ('average', 'hadamard', 'l1', 'l2')
INFO_FIELDS = ('iterations', 'backtracks', 'grad_inf', 'decrement', 'converged', 'degenerate', 'passes', 'loss_evaluations')
MAX_BATCH = 1 << 24


def _op_id(op):
    if isinstance(op, str):
        if op not in OPERATORS:
            raise ValueError('operator %r: one of %s' % (op, ', '.join(FEATURE_OPS)))
        return OPERATORS[op]
    return int(op)


def _pair_keys(n, st, ed, is_undirected):
    st = np.asarray(st, dtype=np.int64); ed = np.asarray(ed, dtype=np.int64)
    if is_undirected:
        st, ed = np.minimum(st, ed), np.maximum(st, ed)
    return st * n + ed


def _member(sorted_keys, q):
    if sorted_keys.size == 0:
        return np.zeros(len(q), dtype=bool)
    pos = np.minimum(np.searchsorted(sorted_keys, q), sorted_keys.size - 1)
    return sorted_keys[pos] == q


def sample_non_edges(graph, m, seed, is_undirected=True, exclude=None):
    """(st, ed) int32 (m,): m distinct node pairs of `graph` that are not arcs, uniform over the pairs u != v, on RandomState(seed).
    Undirected: pairs are canonical (u < v) and rejected if either orientation is an arc.  `exclude` = (st, ed): pairs that are rejected too.
    Drawn in batches, duplicates dropped keeping the first occurrence, until there are m.  ValueError when m exceeds half the non-edges that
    exist (outside `exclude`): a dense graph is refused, never sampled for ever."""
    from gem_amd.graph import edge_arrays
    n, src, dst, _, _ = edge_arrays(graph)
    m = int(m)
    if m < 0:
        raise ValueError('m = %d' % m)
    src = np.asarray(src, dtype=np.int64); dst = np.asarray(dst, dtype=np.int64)
    proper = src != dst
    barred = _pair_keys(n, src[proper], dst[proper], is_undirected)
    if exclude is not None:
        ex_st, ex_ed = np.asarray(exclude[0], dtype=np.int64), np.asarray(exclude[1], dtype=np.int64)
        keep = ex_st != ex_ed
        barred = np.concatenate([barred, _pair_keys(n, ex_st[keep], ex_ed[keep], is_undirected)])
    barred = np.unique(barred)
    total = n * (n - 1) // 2 if is_undirected else n * (n - 1)
    free = total - len(barred)
    if m > free // 2:
        raise ValueError('sample_non_edges: %d pairs asked for, %d non-edges exist: at most half of them can be sampled' % (m, free))
    rng = np.random.RandomState(seed)
    got = np.zeros(0, np.int64)
    while len(got) < m:
        accept = max((free - len(got)) / float(max(n, 1)) ** 2, 1e-9)                    # share of an (u, v) draw that is a new non-edge, at least
        batch = int(min(MAX_BATCH, max(1024, 1.25 * (m - len(got)) / accept)))
        u = rng.randint(0, n, size=batch).astype(np.int64); v = rng.randint(0, n, size=batch).astype(np.int64)
        ok = u != v
        key = _pair_keys(n, u[ok], v[ok], is_undirected)
        key = key[~_member(barred, key)]
        key = np.concatenate([got, key])
        _, first = np.unique(key, return_index=True)
        got = key[np.sort(first)]                                                         # first occurrences, in draw order
    got = got[:m]
    return (got // n).astype(np.int32), (got % n).astype(np.int32)


def positive_pairs(graph, is_undirected=True):
    """(st, ed) int32: the arcs of `graph` without self-loops and repeats, ascending by (st, ed); undirected: one orientation each, st < ed."""
    from gem_amd.graph import edge_arrays
    n, src, dst, _, _ = edge_arrays(graph)
    src = np.asarray(src, dtype=np.int64); dst = np.asarray(dst, dtype=np.int64)
    proper = src != dst
    key = np.unique(_pair_keys(n, src[proper], dst[proper], is_undirected))
    return n, (key // n).astype(np.int32), (key % n).astype(np.int32)


def link_pairs(train_graph, test_graph, seed=0, is_undirected=True, neg_ratio=1.0, max_train_pairs=None):
    """The four pair sets of the protocol, host code: {'train': (st, ed, label), 'test': (st, ed, label), counts}.
    Training positives: positive_pairs(train_graph), subsampled to max_train_pairs on RandomState(seed) (kept in ascending order);
    training negatives: round(neg_ratio * positives) non-edges of train + test, sample_non_edges(seed).  Test positives:
    positive_pairs(test_graph) that are not training arcs; test negatives: as many non-edges of train + test, sample_non_edges(seed + 1),
    disjoint from the training negatives.  Each set lists its positives first."""
    from gem_amd.graph import EdgeListGraph, edge_arrays
    n, ptr_st, ptr_ed = positive_pairs(train_graph, is_undirected)
    n_test, pte_st, pte_ed = positive_pairs(test_graph, is_undirected)
    if n_test != n:
        raise ValueError('link_pairs: the train graph has %d nodes, the test graph %d' % (n, n_test))
    in_train = _member(_pair_keys(n, ptr_st, ptr_ed, is_undirected), _pair_keys(n, pte_st, pte_ed, is_undirected))
    pte_st, pte_ed = pte_st[~in_train], pte_ed[~in_train]
    if max_train_pairs is not None and len(ptr_st) > int(max_train_pairs):
        pick = np.sort(np.random.RandomState(seed).choice(len(ptr_st), size=int(max_train_pairs), replace=False))
        ptr_st, ptr_ed = ptr_st[pick], ptr_ed[pick]
    _, rs, rd, _, _ = edge_arrays(train_graph)
    _, ts, td, _, _ = edge_arrays(test_graph)
    union = EdgeListGraph(n, np.concatenate([rs, ts]), np.concatenate([rd, td]))
    ntr_st, ntr_ed = sample_non_edges(union, int(round(neg_ratio * len(ptr_st))), seed, is_undirected)
    nte_st, nte_ed = sample_non_edges(union, len(pte_st), seed + 1, is_undirected, exclude=(ntr_st, ntr_ed))

    def join(ps, pe, ns, ne):
        return (np.concatenate([ps, ns]).astype(np.int32), np.concatenate([pe, ne]).astype(np.int32),
                np.concatenate([np.ones(len(ps), np.uint8), np.zeros(len(ns), np.uint8)]))
    return {'n': n, 'train': join(ptr_st, ptr_ed, ntr_st, ntr_ed), 'test': join(pte_st, pte_ed, nte_st, nte_ed),
            'n_train_pos': len(ptr_st), 'n_train_neg': len(ntr_st), 'n_test_pos': len(pte_st), 'n_test_neg': len(nte_st)}


class EdgeClassifier(DeviceHandle):
    """gemhip_edgeclf_t with its calls; X is uploaded once: `with EdgeClassifier(X) as ec:`."""

    _destroy = 'gemhip_edgeclf_destroy'

    def __init__(self, X, d=None):
        """X (n, ld) float32; d: how many leading columns count (all by default; the rest is padding the device never reads)."""
        DeviceHandle.__init__(self)
        X, self.n, self.d, ld = embedding_matrix(X, d)
        _hip.check(_hip.lib().gemhip_edgeclf_create(self.n, self.d, ld, _hip.ptr(X, ct.c_float), ct.byref(self._h)))

    @staticmethod
    def _pairs(st, ed):
        st = _hip.as_i32(np.asarray(st).ravel()); ed = _hip.as_i32(np.asarray(ed).ravel())
        if st.shape != ed.shape:
            raise ValueError('st and ed must have equal length')
        return st, ed

    def features(self, op, st, ed):
        """float32 (m, d): op(X[st], X[ed]) row by row."""
        st, ed = self._pairs(st, ed)
        F = np.zeros((len(st), self.d), np.float32)
        _hip.check(_hip.lib().gemhip_edgeclf_features(self._h, _op_id(op), len(st), _hip.ptr(st, ct.c_int32), _hip.ptr(ed, ct.c_int32), _hip.ptr(F, ct.c_float)))
        return F

    def fit(self, op, st, ed, label, C=1.0, dec_tol=DEC_TOL, max_iter=MAX_ITER, w0=None, warn=True):
        """-> (w (d + 1,) float64, weights then intercept, info).  label: 0 / 1 per pair.  info: INFO_FIELDS plus the timings of stats()."""
        st, ed = self._pairs(st, ed)
        y = np.ascontiguousarray(np.asarray(label).ravel(), dtype=np.uint8)
        if y.shape != st.shape:
            raise ValueError('label must have one entry per pair')
        w = np.zeros(self.d + 1) if w0 is None else np.array(w0, dtype=np.float64, order='C').ravel()
        if w.shape != (self.d + 1,):
            raise ValueError('w0 must have d + 1 = %d entries' % (self.d + 1))
        raw = np.zeros(8)
        _hip.check(_hip.lib().gemhip_edgeclf_fit(self._h, _op_id(op), len(st), _hip.ptr(st, ct.c_int32), _hip.ptr(ed, ct.c_int32), _hip.ptr(y, ct.c_uint8),
                                                 float(C), float(dec_tol), int(max_iter), _hip.ptr(w, ct.c_double), _hip.ptr(raw, ct.c_double)))
        info = {'iterations': int(raw[0]), 'backtracks': int(raw[1]), 'grad_inf': float(raw[2]), 'decrement': float(raw[3]), 'converged': bool(raw[4]),
                'degenerate': int(raw[5]), 'passes': int(raw[6]), 'loss_evaluations': int(raw[7])}
        info.update(self.stats())
        if warn and not info['converged']:
            warnings.warn('link classification: the fit did not converge in %d iterations (decrement %.2e, |g|_inf %.2e); raise max_iter or dec_tol'
                          % (max_iter, info['decrement'], info['grad_inf']), RuntimeWarning, stacklevel=2)
        return w, info

    def decision_function(self, op, st, ed, w):
        """float64 (m,): the logits sum_j op(X[st], X[ed])_j * w[j] + w[d], no feature matrix formed."""
        st, ed = self._pairs(st, ed)
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
        if w.shape != (self.d + 1,):
            raise ValueError('w must have d + 1 = %d entries' % (self.d + 1))
        out = np.zeros(len(st))
        _hip.check(_hip.lib().gemhip_edgeclf_scores(self._h, _op_id(op), len(st), _hip.ptr(st, ct.c_int32), _hip.ptr(ed, ct.c_int32), _hip.ptr(w, ct.c_double),
                                                    _hip.ptr(out, ct.c_double)))
        return out

    def dot(self, st, ed):
        """float64 (m,): X[st] . X[ed], fp64 sums of the float32 rows -- the baseline without a classifier."""
        st, ed = self._pairs(st, ed)
        out = np.zeros(len(st))
        _hip.check(_hip.lib().gemhip_edgeclf_scores(self._h, 0, len(st), _hip.ptr(st, ct.c_int32), _hip.ptr(ed, ct.c_int32), None, _hip.ptr(out, ct.c_double)))
        return out

    def stats(self):
        ms = (ct.c_double * 6)(); out = (ct.c_int64 * 8)()
        _hip.check(_hip.lib().gemhip_edgeclf_last_ms(self._h, ms))
        _hip.check(_hip.lib().gemhip_edgeclf_info(self._h, out))
        return {'upload_ms': ms[0], 'features_ms': ms[1], 'scores_ms': ms[2], 'fit_ms': ms[3], 'pass_ms': ms[4], 'fit_features_ms': ms[5],
                'pairs_per_wave': int(out[2]), 'pairs_per_workgroup': int(out[3]), 'newton_iterations': int(out[6])}


def _score_pairs(ec, pairs, op, C, graph_embedding, X, test_graph, train_graph=None):
    """(scores of the test pairs, w or None, info or None, fit seconds, scoring seconds).  train_graph: the graph a neighbourhood score
    (HEURISTICS) is computed on, or an open NeighbourScorer of it; ec and X are not consulted then."""
    st, ed, _ = pairs['test']
    t0 = time.perf_counter()
    w = info = None
    if op in OPERATORS:
        w, info = ec.fit(op, *pairs['train'], C=C)
    t1 = time.perf_counter()
    if op in OPERATORS:
        score = ec.decision_function(op, st, ed, w)
    elif op == 'dot':
        score = ec.dot(st, ed)
    elif op == 'method':
        if graph_embedding is None:
            raise ValueError("op='method' needs graph_embedding")
        from gem_amd.evaluation.reconstruction import _DeviceEvaluator
        from gem_amd.graph import edge_arrays
        n, tsrc, tdst, _, _ = edge_arrays(test_graph)
        with _DeviceEvaluator(n, tsrc, tdst, graph_embedding, X) as ev:
            score, _ = ev.pairs(st, ed, want_hit=False)
    elif op in HEURISTICS:
        if train_graph is None:
            raise ValueError('op=%r needs train_graph' % (op,))
        if isinstance(train_graph, NeighbourScorer):
            score = train_graph.scores(st, ed, (op,))[op]
        else:
            with NeighbourScorer(train_graph) as ns:
                score = ns.scores(st, ed, (op,))[op]
        score = np.asarray(score, dtype=np.float64)
    else:
        raise ValueError("op = %r: one of %s, 'dot', 'method'; or a neighbourhood score without an embedding: %s" % (op, ', '.join(FEATURE_OPS), ', '.join(HEURISTICS)))
    return score, w, info, t1 - t0, time.perf_counter() - t1


def _evaluate(ec, pairs, op, C, graph_embedding, X, test_graph, sample_s, train_graph=None):
    score, w, info, fit_s, score_s = _score_pairs(ec, pairs, op, C, graph_embedding, X, test_graph, train_graph)
    t0 = time.perf_counter()
    res = ranking.binary_ranking_scores(score, pairs['test'][2])
    rank_s = time.perf_counter() - t0
    out = {'auc': res['auc'], 'ap': res['ap'], 'op': op, 'coef': w, 'info': info, 'n_thresholds': res['n_thresholds'], 'sample_s': sample_s, 'fit_s': fit_s,
           'score_s': score_s, 'rank_s': rank_s}
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        out[k] = pairs[k]
    return out


def evaluate_link_classification(train_graph, test_graph, X, op='hadamard', C=1.0, seed=0, is_undirected=True, neg_ratio=1.0, max_train_pairs=None,
                                 graph_embedding=None):
    """One run of the protocol for the embedding X (n, d) trained on train_graph: link_pairs(...) makes the pair sets, the classifier of `op`
    is fitted on the training pairs and the test pairs are ranked.  op: 'average', 'hadamard', 'l1', 'l2'; 'dot' (no fit); 'method'
    (graph_embedding's own edge weight, through the evaluator's pair scores); 'cn', 'jaccard', 'aa', 'ra', 'pa' (link_heuristics: the
    neighbourhood score on train_graph, no fit, X is not consulted and may be None).  Returns a dict: 'auc', 'ap', the four pair counts, 'coef'
    ((d + 1,) weights then intercept, None without a fit), 'info' (EdgeClassifier.fit's), 'n_thresholds', and the seconds spent sampling,
    fitting, scoring and ranking."""
    _hip.require_device()
    t0 = time.perf_counter()
    pairs = link_pairs(train_graph, test_graph, seed, is_undirected, neg_ratio, max_train_pairs)
    sample_s = time.perf_counter() - t0
    if op in HEURISTICS:
        return _evaluate(None, pairs, op, C, graph_embedding, X, test_graph, sample_s, train_graph)
    X = np.asarray(X)
    if X.shape[0] != pairs['n']:
        raise ValueError('embedding has %d rows, the graphs %d nodes' % (X.shape[0], pairs['n']))
    with EdgeClassifier(X) as ec:
        return _evaluate(ec, pairs, op, C, graph_embedding, X, test_graph, sample_s)


def _split_and_embed(digraph, graph_embedding, train_ratio, is_undirected, lcc):
    from gem_amd.evaluation.link_prediction import restrict_to_train_lcc
    from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
    train, test = split_di_graph_to_train_test(digraph, train_ratio, is_undirected)
    if lcc:
        train, test, _ = restrict_to_train_lcc(train, test)
    X = graph_embedding.learn_embedding(graph=train, no_python=True)
    if isinstance(X, tuple):
        X = X[0]
    return train, test, np.asarray(X)


def evaluateStaticLinkClassification(digraph, graph_embedding, train_ratio=0.8, op='hadamard', lcc=False, is_undirected=True, C=1.0, seed=0, neg_ratio=1.0,
                                     max_train_pairs=None):
    """Split `digraph` (split_di_graph_to_train_test: numpy's global stream, so np.random.seed reproduces the split), with lcc=True cut both
    graphs down to the train graph's largest component (restrict_to_train_lcc), train `graph_embedding` on the train graph and run
    evaluate_link_classification.  Returns its dict."""
    train, test, X = _split_and_embed(digraph, graph_embedding, train_ratio, is_undirected, lcc)
    return evaluate_link_classification(train, test, X, op=op, C=C, seed=seed, is_undirected=is_undirected, neg_ratio=neg_ratio, max_train_pairs=max_train_pairs,
                                        graph_embedding=graph_embedding)


def expLinkClassification(digraph, graph_embedding, rounds, ops=FEATURE_OPS, train_ratio=0.8, lcc=False, is_undirected=True, C=1.0, seed=0, neg_ratio=1.0,
                          max_train_pairs=None):
    """Every operator x round: {op: {'auc': [...], 'ap': [...]}}.  Round r seeds numpy's global stream with seed + r for the split, trains the
    embedding once, builds the pair sets once (link_pairs(seed + r)) and keeps X on the device for all operators.  `ops` may name neighbourhood
    scores too -- ops=('hadamard', 'dot', 'cn', 'aa') is table 4 from one set of pairs."""
    _hip.require_device()
    out = {op: {'auc': [], 'ap': []} for op in ops}
    for r in range(rounds):
        np.random.seed(seed + r)
        train, test, X = _split_and_embed(digraph, graph_embedding, train_ratio, is_undirected, lcc)
        t0 = time.perf_counter()
        pairs = link_pairs(train, test, seed + r, is_undirected, neg_ratio, max_train_pairs)
        sample_s = time.perf_counter() - t0
        ns = NeighbourScorer(train) if any(op in HEURISTICS for op in ops) else None          # the train graph is ingested once per round
        try:
            with EdgeClassifier(X) as ec:
                for op in ops:
                    res = _evaluate(ec, pairs, op, C, graph_embedding, X, test, sample_s, ns)
                    out[op]['auc'].append(res['auc']); out[op]['ap'].append(res['ap'])
        finally:
            if ns is not None:
                ns.close()
    return out
