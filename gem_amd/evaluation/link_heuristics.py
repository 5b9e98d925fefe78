"""The neighbourhood baselines of link prediction on the GPU (gem_amd/csrc/nbr.hip): common neighbours, Jaccard's
coefficient, Adamic-Adar, resource allocation and preferential attachment -- the first rows of the node2vec paper's table 4, the scores every
AUC of an embedding is compared with.  All five are defined on the simple undirected graph of the input (both orientations merged,
self-loops and repeats dropped, weights ignored), as networkx's functions on an nx.Graph.  The pair protocol is link_classification's
(link_pairs): the test pairs are scored on the TRAIN graph and ranked by ranking.binary_ranking_scores; no embedding is trained and nothing is
fitted.  The graph is ingested on the host; the scores run on the device.  No host fallback: GemHipError without a device."""
import ctypes as ct
import time

import numpy as np

from gem_amd import _hip
from gem_amd.evaluation import ranking
from gem_amd.evaluation._handle import DeviceHandle

HEURISTICS = ('cn', 'jaccard', 'aa', 'ra', 'pa')
_BIT = {'cn': 1, 'jaccard': 2, 'aa': 4, 'ra': 8, 'pa': 16}
_TABLE = {'aa': 0, 'ra': 1}


def _names(which):
    which = (which,) if isinstance(which, str) else tuple(which)
    for name in which:
        if name not in _BIT:
            raise ValueError('heuristic %r: one of %s' % (name, ', '.join(HEURISTICS)))
    if not which:
        raise ValueError('no heuristic asked for: some of %s' % ', '.join(HEURISTICS))
    return which


def constants():
    """{'lanes_per_narrow_group', 'narrow', 'chunk'}: the planner's constants (gemhip_nbr_info); no device needed."""
    out = (ct.c_int64 * 12)()
    _hip.check(_hip.lib().gemhip_nbr_info(None, out))
    return {'lanes_per_narrow_group': int(out[3]), 'narrow': int(out[4]), 'chunk': int(out[5])}


class NeighbourScorer(DeviceHandle):
    """gemhip_nbr_t with its calls; the graph is ingested and uploaded once: `with NeighbourScorer(graph) as ns:`."""

    _destroy = 'gemhip_nbr_destroy'

    def __init__(self, graph):
        """graph: anything gem_amd.graph.edge_arrays accepts (an nx graph with node ids 0 .. n-1, an EdgeListGraph)."""
        from gem_amd.graph import edge_arrays
        DeviceHandle.__init__(self)
        n, src, dst, _, _ = edge_arrays(graph)
        src = _hip.as_i32(src); dst = _hip.as_i32(dst)
        self.n = int(n)
        _hip.check(_hip.lib().gemhip_nbr_create(self.n, len(src), _hip.ptr(src, ct.c_int32), _hip.ptr(dst, ct.c_int32), ct.byref(self._h)))

    def degrees(self):
        """int32 (n,): the degrees in the simple undirected graph."""
        deg = np.zeros(self.n, np.int32)
        _hip.check(_hip.lib().gemhip_nbr_degrees(self._h, _hip.ptr(deg, ct.c_int32)))
        return deg

    def weights(self, which):
        """float64 (n,): the table the kernel gathers, read back from the device: 'aa' 1 / ln(deg), 'ra' 1 / deg."""
        if which not in _TABLE:
            raise ValueError("weights %r: 'aa' or 'ra'" % (which,))
        w = np.zeros(self.n)
        _hip.check(_hip.lib().gemhip_nbr_weights(self._h, _TABLE[which], _hip.ptr(w, ct.c_double)))
        return w

    def scores(self, st, ed, which=HEURISTICS):
        """{name: (m,) array}: 'cn' int32, the others float64.  st != ed; repeated and adjacent pairs are legal."""
        which = _names(which)
        st = _hip.as_i32(np.asarray(st).ravel()); ed = _hip.as_i32(np.asarray(ed).ravel())
        if st.shape != ed.shape:
            raise ValueError('st and ed must have equal length')
        out = {name: np.zeros(len(st), np.int32 if name == 'cn' else np.float64) for name in which}
        mask = sum(_BIT[name] for name in set(which))
        _hip.check(_hip.lib().gemhip_nbr_scores(self._h, len(st), _hip.ptr(st, ct.c_int32), _hip.ptr(ed, ct.c_int32), mask, _hip.ptr(out.get('cn'), ct.c_int32),
                                                *[_hip.ptr(out.get(name), ct.c_double) for name in HEURISTICS[1:]]))
        return out

    def stats(self):
        ms = (ct.c_double * 6)(); out = (ct.c_int64 * 12)()
        _hip.check(_hip.lib().gemhip_nbr_last_ms(self._h, ms))
        _hip.check(_hip.lib().gemhip_nbr_info(self._h, out))
        return {'ingest_ms': ms[0], 'graph_upload_ms': ms[1], 'plan_ms': ms[2], 'pair_upload_ms': ms[3], 'kernel_ms': ms[4], 'download_ms': ms[5],
                'n': int(out[0]), 'stored_neighbours': int(out[1]), 'max_degree': int(out[2]), 'lanes_per_narrow_group': int(out[3]), 'narrow': int(out[4]),
                'chunk': int(out[5]), 'narrow_items': int(out[6]), 'wide_items': int(out[7]), 'split_pairs': int(out[8]), 'partial_slots': int(out[9]),
                'longest_item': int(out[10]), 'pairs': int(out[11])}


def _rank(score, pairs, sample_s, ingest_s, score_s):
    t0 = time.perf_counter()
    res = {}
    for name, s in score.items():
        r = ranking.binary_ranking_scores(np.asarray(s, dtype=np.float64), pairs['test'][2])
        res[name] = {'auc': r['auc'], 'ap': r['ap'], 'n_thresholds': r['n_thresholds']}
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        res[k] = pairs[k]
    res.update({'sample_s': sample_s, 'ingest_s': ingest_s, 'score_s': score_s, 'rank_s': time.perf_counter() - t0})
    return res


def evaluate_link_heuristics(train_graph, test_graph, which=HEURISTICS, seed=0, is_undirected=True, neg_ratio=1.0):
    """One run of link_classification's protocol without an embedding: link_pairs(...) makes the pair sets exactly as there, the test pairs
    are scored on the TRAIN graph and ranked.  Returns {name: {'auc', 'ap', 'n_thresholds'}} for every name in `which`, the four pair counts
    and the seconds spent sampling, ingesting (host CSR and upload), scoring and ranking."""
    from gem_amd.evaluation.link_classification import link_pairs
    which = _names(which)
    _hip.require_device()
    t0 = time.perf_counter()
    pairs = link_pairs(train_graph, test_graph, seed, is_undirected, neg_ratio)
    t1 = time.perf_counter()
    with NeighbourScorer(train_graph) as ns:
        t2 = time.perf_counter()
        score = ns.scores(pairs['test'][0], pairs['test'][1], which)
        t3 = time.perf_counter()
    return _rank(score, pairs, t1 - t0, t2 - t1, t3 - t2)


def evaluateStaticLinkHeuristics(digraph, train_ratio=0.8, which=HEURISTICS, lcc=False, is_undirected=True, seed=0, neg_ratio=1.0):
    """Split `digraph` as evaluateStaticLinkClassification does (split_di_graph_to_train_test on numpy's global stream; lcc=True cuts both
    graphs down to the train graph's largest component) and run evaluate_link_heuristics.  Returns its dict."""
    from gem_amd.evaluation.link_prediction import restrict_to_train_lcc
    from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
    _hip.require_device()
    train, test = split_di_graph_to_train_test(digraph, train_ratio, is_undirected)
    if lcc:
        train, test, _ = restrict_to_train_lcc(train, test)
    return evaluate_link_heuristics(train, test, which=which, seed=seed, is_undirected=is_undirected, neg_ratio=neg_ratio)


def expLinkHeuristics(digraph, rounds, which=HEURISTICS, train_ratio=0.8, lcc=False, is_undirected=True, seed=0, neg_ratio=1.0):
    """Every heuristic x round: {name: {'auc': [...], 'ap': [...]}}.  Round r seeds numpy's global stream with seed + r for the split and
    builds the pair sets with link_pairs(seed + r), as expLinkClassification does: the same seeds give the same pairs."""
    which = _names(which)
    _hip.require_device()
    out = {name: {'auc': [], 'ap': []} for name in which}
    for r in range(rounds):
        np.random.seed(seed + r)
        res = evaluateStaticLinkHeuristics(digraph, train_ratio, which, lcc, is_undirected, seed + r, neg_ratio)
        for name in which:
            out[name]['auc'].append(res[name]['auc']); out[name]['ap'].append(res[name]['ap'])
    return out
