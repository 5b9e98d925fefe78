"""GPU tier of the neighbourhood link-prediction baselines (gem_amd/csrc/nbr.hip): the five scores against tests/nbr_refs.py on hand graphs,
on two-hub graphs whose list lengths straddle every constant of the planner, on mixed batches of a power-law graph and on the SBM-1024 link
fixture; the protocol end to end against the networkx / sklearn golden; determinism.  cn, jaccard and pa are compared with ==; an fp64 sum
against math.fsum over the weight table read back from the device, within (k + 1) 2^-53 of it (k - 1 additions in any order of positive
terms, and fsum's own rounding).  Nothing here provokes a fault: every refusal is decided on the host before a launch."""
import json

import numpy as np
import pytest

import nbr_refs as NB
import rank_refs as R
from conftest import golden_path
from gem_amd import _hip
from gem_amd.evaluation import link_classification as LC
from gem_amd.evaluation import link_heuristics as LH
from gem_amd.graph import EdgeListGraph, rmat_graph

pytestmark = pytest.mark.gpu

LANES, NARROW, CHUNK = NB.LANES, NB.NARROW, NB.CHUNK
ULP = 2.0 ** -52


def check_scores(ns, A, st, ed, got=None):
    """All five scores of the pairs against the restatements; returns the device's dict."""
    got = ns.scores(st, ed) if got is None else got
    ref = NB.scores(A, st, ed)
    assert got['cn'].dtype == np.int32 and all(got[k].dtype == np.float64 for k in ('jaccard', 'aa', 'ra', 'pa'))
    for name in ('cn', 'jaccard', 'pa'):
        assert np.array_equal(got[name], ref[name]), name
    for name in ('aa', 'ra'):
        exact = NB.fsum_scores(ns.weights(name), A, st, ed)
        assert np.all(np.abs(got[name] - exact) <= NB.sum_bound(ref['cn'], exact)), name
        assert np.all(got[name][ref['cn'] == 0] == 0.0)
    stats = ns.stats()
    assert (stats['narrow_items'], stats['wide_items'], stats['split_pairs'], stats['partial_slots']) == NB.plan_counts(NB.degrees(A), st, ed)
    return got


def test_kernel_constants_are_the_ones_the_shapes_below_were_chosen_for():
    with LH.NeighbourScorer(EdgeListGraph(3, [0, 1], [1, 2])) as ns:
        st = ns.stats()
        assert (st['lanes_per_narrow_group'], st['narrow'], st['chunk']) == (16, 32, 2048) == (LANES, NARROW, CHUNK)
        assert (st['n'], st['stored_neighbours'], st['max_degree']) == (3, 4, 2)
        assert np.array_equal(ns.degrees(), [1, 2, 1])
        w_aa, w_ra = NB.weight_tables(np.array([1, 2, 1]))
        assert np.array_equal(ns.weights('aa'), w_aa) and np.array_equal(ns.weights('ra'), w_ra)


def test_hand_graph():
    n, src, dst = NB.hand_graph()
    A = NB.simple_csr(n, src, dst)
    st = np.array([9, 11, 4, 0, 0, 6, 6, 7, 0, 1, 6, 0, 11], np.int32)
    ed = np.array([5, 0, 11, 1, 2, 7, 7, 6, 6, 0, 8, 9, 3], np.int32)
    with LH.NeighbourScorer(EdgeListGraph(n, src, dst)) as ns:
        got = check_scores(ns, A, st, ed)
    row = {k: got[k].tolist() for k in got}
    assert row['cn'][0] == 0 and row['jaccard'][0] == 0.0 and row['pa'][0] == 3.0                 # an empty intersection of non-empty lists
    assert row['jaccard'][1] == 0.0 and row['pa'][1] == 0.0 and row['pa'][2] == 0.0               # a degree-0 endpoint, either side
    assert row['cn'][3] == 1 and row['jaccard'][3] == 1.0 / 5.0                                   # adjacent, in the triangle: v counts in the union only
    assert row['cn'][5] == 2 and row['jaccard'][5] == 1.0 and row['ra'][5] == 1.0 / 4.0 + 1.0 / 3.0      # 6 and 7: both tied to 1 (degree 4) and 5 (degree 3)
    for k in got:
        assert got[k][5] == got[k][6] == got[k][7]                                                # the same pair twice, and in the other orientation
        assert got[k][3] == got[k][9]
    assert row['cn'][12] == 0 and row['jaccard'][12] == 0.0


LA = [1, 15, 16, 17, NARROW - 1, NARROW, NARROW + 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]


@pytest.mark.parametrize('la', LA)
def test_two_hub_graph_every_length_and_overlap(la):
    rng = np.random.RandomState(la)
    for lb in (la, la + 1, 4 * la + 5):
        for overlap in sorted({0, 1, la // 2, la}):
            n, src, dst, a, b = NB.two_hub_graph(la, lb, overlap)
            A = NB.simple_csr(n, src, dst)
            small = np.arange(10, n) if n - 10 >= 2 else np.arange(2, n)                          # leaves and shared nodes: degree <= 9, narrow pairs
            u = rng.choice(small, size=8); v = rng.choice(small, size=8)
            v = np.where(u == v, small[(np.searchsorted(small, u) + 1) % len(small)], v)
            # the hub pair first, between narrow pairs of one wave, in the other orientation, and last; two filler nodes (long lists when the overlap is)
            st = np.concatenate([[a], u[:2], [a], u[2:], [b, 2], [a]]).astype(np.int32)
            ed = np.concatenate([[b], v[:2], [b], v[2:], [a, 3], [b]]).astype(np.int32)
            with LH.NeighbourScorer(EdgeListGraph(n, src, dst)) as ns:
                assert np.array_equal(ns.degrees(), NB.degrees(A))
                got = check_scores(ns, A, st, ed)
                alone = ns.scores([a], [b])
            assert got['cn'][0] == overlap and got['pa'][0] == float(la) * float(lb)
            for k in got:
                assert got[k][0] == got[k][3] == got[k][-3] == got[k][-1] == alone[k][0], (k, lb, overlap)


@pytest.fixture(scope='module')
def rmat():
    g = rmat_graph(12, 65536, 7)
    A = NB.simple_csr(g.n, g.src, g.dst)
    return g, A, NB.degrees(A)


@pytest.mark.parametrize('m', [1, 3, 4, 5, 257, 4099])
def test_mixed_batches_of_a_power_law_graph(m, rmat):
    g, A, deg = rmat
    rng = np.random.RandomState(m)
    hubs = np.argsort(-deg, kind='stable')[:64]
    assert deg[hubs[0]] > NARROW and (deg == 0).any() and (deg[deg > 0] <= NARROW).any()
    st = np.where(rng.random_sample(m) < 0.3, rng.choice(hubs, size=m), rng.randint(0, g.n, size=m))           # hubs and leaves share waves
    ed = np.where(rng.random_sample(m) < 0.3, rng.choice(hubs, size=m), rng.randint(0, g.n, size=m))
    ed = np.where(st == ed, (ed + 1) % g.n, ed)
    with LH.NeighbourScorer(g) as ns:
        check_scores(ns, A, st.astype(np.int32), ed.astype(np.int32))


def test_a_batch_without_any_item_is_still_written(rmat):
    g, A, deg = rmat
    lone = np.flatnonzero(deg == 0)
    some = np.flatnonzero(deg > 0)
    assert len(lone) >= 2
    st = np.concatenate([lone[:1], some[:70], lone[:1]]).astype(np.int32)
    ed = np.concatenate([lone[1:2], np.full(70, lone[0]), some[:1]]).astype(np.int32)
    with LH.NeighbourScorer(g) as ns:
        ns.scores(some[:100], some[100:200])                                                                  # the buffers now hold other values
        got = check_scores(ns, A, st, ed)
        stats = ns.stats()
    assert stats['narrow_items'] == stats['wide_items'] == stats['split_pairs'] == 0 and stats['pairs'] == len(st)
    assert not got['cn'].any() and not any(got[k].any() for k in ('jaccard', 'aa', 'ra', 'pa'))


@pytest.fixture(scope='module')
def split():
    train, test, pairs = R.fixture_pairs()
    return train, test, pairs, NB.simple_csr(train.n, train.src, train.dst)


@pytest.fixture(scope='module')
def device_scores(split):
    train, _, pairs, _ = split
    with LH.NeighbourScorer(train) as ns:
        return ns.scores(pairs['test'][0], pairs['test'][1])


def test_fixture_pairs_all_five_scores(split, device_scores):
    train, _, pairs, A = split
    with LH.NeighbourScorer(train) as ns:
        check_scores(ns, A, pairs['test'][0], pairs['test'][1])
    ref = NB.scores(A, pairs['test'][0], pairs['test'][1])
    assert all(np.array_equal(device_scores[k], ref[k]) for k in ('cn', 'jaccard', 'pa'))


@pytest.fixture(scope='module')
def protocol(split):
    train, test, _, _ = split
    return LH.evaluate_link_heuristics(train, test, seed=R.PAIR_SEED)


def test_protocol_end_to_end_against_the_golden(split, protocol, device_scores):
    _, _, pairs, _ = split
    meta = json.load(open(golden_path('link_baselines_ref.json')))
    tol = 4 * json.load(open(golden_path('link_auc_ref.json')))['sklearn_metrics_vs_exact']
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        assert protocol[k] == meta[k] == pairs[k]
    P, N = protocol['n_test_pos'], protocol['n_test_neg']
    for name in LH.HEURISTICS:
        res, entry = protocol[name], meta['heuristics'][name]
        if name in ('aa', 'ra'):
            auc_bound = entry['near'] / float(P * N) + ULP
            ap_bound = entry['ap_sensitivity'] + 4 * entry['n_thresholds'] * 2.0 ** -53
        else:
            auc_bound = ap_bound = tol
        print('%s: auc %.12f (golden %.12f, |diff| %.2e, bound %.2e)  ap %.12f (golden %.12f, |diff| %.2e, bound %.2e)' %
              (name, res['auc'], entry['auc'], abs(res['auc'] - entry['auc']), auc_bound, res['ap'], entry['ap'], abs(res['ap'] - entry['ap']), ap_bound))
        assert abs(res['auc'] - entry['auc']) <= auc_bound
        assert abs(res['ap'] - entry['ap']) <= ap_bound
        ex = R.exact_scores(device_scores[name].astype(np.float64), pairs['test'][2])                  # the metrics of the scores the device returned
        assert res['n_thresholds'] == ex['T']
        assert abs(res['auc'] - float(ex['auc'])) <= ULP * float(ex['auc'])
        assert abs(res['ap'] - float(ex['ap'])) <= 4 * ex['T'] * 2.0 ** -53 * float(ex['ap'])
        if name not in ('aa', 'ra'):
            assert res['n_thresholds'] == entry['n_thresholds']
    for k in ('sample_s', 'ingest_s', 'score_s', 'rank_s'):
        assert protocol[k] >= 0.0


def test_link_classification_accepts_the_heuristics_as_op(split, protocol):
    train, test, _, _ = split
    res = LC.evaluate_link_classification(train, test, None, op='aa', seed=R.PAIR_SEED)
    assert res['coef'] is None and res['info'] is None and res['op'] == 'aa'
    assert (res['auc'], res['ap'], res['n_thresholds']) == (protocol['aa']['auc'], protocol['aa']['ap'], protocol['aa']['n_thresholds'])
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        assert res[k] == protocol[k]
    with pytest.raises(_hip.GemHipError, match=r'pair 1 = \(3,3\): st == ed'):
        with LH.NeighbourScorer(train) as ns:
            ns.scores([0, 3], [1, 3])


def test_two_calls_give_identical_bytes_and_a_subset_equals_the_full_call(split, device_scores, rmat):
    train, _, pairs, _ = split
    st, ed, _ = pairs['test']
    with LH.NeighbourScorer(train) as ns:
        again = ns.scores(st, ed)
        part = ns.scores(st, ed, ('ra', 'cn'))
        one = ns.scores(st, ed, 'jaccard')
        swapped = ns.scores(ed, st)
    assert set(part) == {'ra', 'cn'} and set(one) == {'jaccard'}
    for k in LH.HEURISTICS:
        assert again[k].tobytes() == device_scores[k].tobytes() == swapped[k].tobytes(), k
    assert part['ra'].tobytes() == device_scores['ra'].tobytes() and part['cn'].tobytes() == device_scores['cn'].tobytes()
    assert one['jaccard'].tobytes() == device_scores['jaccard'].tobytes()
    g, _, deg = rmat                                                                                    # long lists: split pairs and wide items too
    hubs = np.argsort(-deg, kind='stable')[:40]
    with LH.NeighbourScorer(g) as ns:
        a = ns.scores(hubs[:20], hubs[20:]); b = ns.scores(hubs[:20], hubs[20:]); c = ns.scores(hubs[20:], hubs[:20])
    assert all(a[k].tobytes() == b[k].tobytes() == c[k].tobytes() for k in LH.HEURISTICS)
