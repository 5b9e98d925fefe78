"""GPU tests of the partitioned (multi-GPU episode) SGNS path -- gemhip_sgns_train_part, the walk-ordered bucket kernel -- and of the 16k-node parity point."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import oracle
from gem_amd import _hip, multi_gpu
from gem_amd.embedding.node2vec import node2vec
from gem_amd.evaluation import reconstruction as gr
from gem_amd.graph import edge_arrays, sbm_graph, to_csr
from conftest import golden_path

pytestmark = pytest.mark.gpu


def backend(G, d):
    n, src, dst, w, _ = edge_arrays(G)
    row_ptr, col, ww = to_csr(n, src, dst, w)
    return n, src, dst, multi_gpu.HipBackendN2V(n, row_ptr, col, ww, d)


def _walks_of(b, l):
    nw = C.c_int64(); wl = C.c_int32(); p = C.c_void_p()
    _hip.check(b.L.gemhip_n2v_walks_ptr(b.h, C.byref(p), C.byref(nw), C.byref(wl)))
    walks = np.empty((nw.value, l), np.int32)
    _hip.check(b.L.gemhip_n2v_get_walks(b.h, _hip.ptr(walks, C.c_int32)))
    return walks


HOT_THR = 15       # corpus of the bucket tests (SBM-1024, walks 100..356 of 40 tokens, seed 3): largest token count 23, mean 10


def _bucket_case(sbm1024, d, parts, bucket, flags, hogwild_path, segments, fresh=0, local_key=False):
    """One bucket launch on ONE wavefront against oracle_sgns_train_part (see the tests below).  hogwild_path 9: hot rows from HOT_THR tokens on, with the
    fresh bits `fresh`; local_key: the hot nodes carry the key INT32_MAX in the count buffer instead (threshold INT32_MAX).  Before a launch with hot rows
    the pairs of the bucket are classified on the CPU (tests/sgns_path_refs.py): at least 5 % of them in each class the case is there for."""
    import sgns_path_refs as spr
    n, src, dst, b = backend(sbm1024, d)
    l = 40
    b.walks(1.0, 1.0, 1, l, 3, flags, 100, 356)
    walks = _walks_of(b, l)
    b.vocab(); b.build_unigram_parts(parts)
    counts = b.counts.cpu().numpy().copy()
    UT, KT, off = oracle.unigram_build_parts(counts, parts)
    UTd = np.empty(n, np.float32); KTd = np.empty(n, np.int32)
    _hip.check(b.L.gemhip_n2v_build_unigram_parts(b.h, parts, _hip.ptr(UTd, C.c_float), _hip.ptr(KTd, C.c_int32)))
    assert np.array_equal(UTd, UT) and np.array_equal(KTd, KT)
    gi, gj = bucket
    P, _, _ = b.init_part_tables(3, gi, parts)
    rows = P.shape[0]
    Np = (0.05 * torch.randn((rows, d), generator=torch.Generator().manual_seed(1))).to(P.device)
    Po, No = P.cpu().numpy().copy(), Np.cpu().numpy().copy()
    thr = 0
    if hogwild_path:
        _hip.check(b.L.gemhip_sgns_set_window_cache(b.h, -1, 1))
        if hogwild_path == 9:
            assert counts.max() == 23 and HOT_THR < counts.max()
            thr = spr.INT32_MAX if local_key else HOT_THR
            key = np.where(counts >= HOT_THR, spr.INT32_MAX, counts).astype(np.int32) if local_key else counts
            wids = np.concatenate([100 + np.arange(150), 250 + np.arange(106)]) if segments else 100 + np.arange(256)
            cls = spr.pair_classes(walks, 5, 3, 0, UT[off[gj]:off[gj + 1]], KT[off[gj]:off[gj + 1]], off[gj + 1] - off[gj], key, thr, fresh=fresh, flags=flags,
                                   wids=wids, bucket=(parts, gi, gj))
            s = spr.assert_floors(cls, ('fast_hot', 'fast_cold', 'slow', 'hot_ctx') + (('hot_word',) if (fresh & 1) or local_key else ()))
            print({k: round(float(v), 4) for k, v in s.items()})
            if local_key:      # the key a Hogwild launch would see, in the buffer the library reads the counts from (the tables above were built from the counts)
                b.counts.copy_(torch.from_numpy(key)); torch.cuda.synchronize()
            _hip.check(b.L.gemhip_sgns_set_hot_rows(b.h, thr))
            _hip.check(b.L.gemhip_sgns_set_fresh(b.h, fresh))
    dev = P.device
    if segments:      # shard 0 = walks [0, 150) with ids 100.., shard 1 = walks [150, 256) with ids 250..; work items 2 x 150 (44 of them absent)
        corpus = torch.from_numpy(walks).to(dev)
        tab = torch.tensor([[[0, 150], [150, 106], [100, 250]]], dtype=torch.int64, device=dev)
        b.train_part(corpus, tab, 0, 2, 150, 5, 0.025, 2 * 150 * l, 1000, 0, 3, flags | 4, gi, gj, P, Np)
        want_pairs = 0
        for r, (lo, cnt, wid0) in enumerate(((0, 150, 100), (150, 106, 250))):
            want_pairs += oracle.sgns_train_part(walks[lo:lo + cnt], None, 5, 0.025, 2 * 150 * l, 1000 + r * 150 * l, 0, parts, gi, gj, UT[off[gj]:off[gj + 1]],
                                                 KT[off[gj]:off[gj + 1]], 3, flags, Po, No, walk_id_offset=wid0, local_rows=True)
    else:
        corpus = torch.from_numpy(walks).to(dev)
        _hip.check(b.L.gemhip_sgns_train_part(b.h, C.c_void_p(corpus.data_ptr()), 256, l, None, 0, 0, 100, 5, 0.025, 256 * l, 0, 0, 3, flags | 4, gi, gj,
                                              C.c_void_p(P.data_ptr()), C.c_void_p(Np.data_ptr()), d, None))
        want_pairs = oracle.sgns_train_part(walks, None, 5, 0.025, 256 * l, 0, 0, parts, gi, gj, UT[off[gj]:off[gj + 1]], KT[off[gj]:off[gj + 1]], 3, flags,
                                            Po, No, walk_id_offset=100, local_rows=True)
    torch.cuda.synchronize()
    if hogwild_path:
        k, wv, hot, fr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _hip.check(b.L.gemhip_sgns_last_launch(b.h, C.byref(k), C.byref(wv), C.byref(hot), C.byref(fr)))
        assert (k.value, wv.value, hot.value, fr.value) == (2, 1, thr, fresh if thr else 0)
    assert b.pairs() == want_pairs > 100
    if thr:
        assert want_pairs == s['pairs']
    for got, want in ((P.cpu().numpy(), Po), (Np.cpu().numpy(), No)):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print('max|got - want| = %.3e, bar %.3e' % (err, 2e-4 * scale + 1e-6))
        assert err <= 2e-4 * scale + 1e-6
    b.close()


@pytest.mark.parametrize('d,parts,bucket,flags,hogwild_path,segments', [(16, 4, (1, 0), 9, 0, False), (128, 2, (0, 1), 11, 0, False), (7, 3, (2, 2), 9, 0, True),
                                                                      (128, 2, (1, 1), 11, 1, True), (64, 5, (3, 1), 11, 9, False), (129, 2, (0, 1), 11, 1, False)])
def test_train_part_deterministic_matches_oracle(sbm1024, d, parts, bucket, flags, hogwild_path, segments):
    """gemhip_sgns_train_part (sgns_win_kernel<PART>) on ONE wavefront == TrainModel in walk order restricted to the bucket (context partition,
    word partition) -- oracle_sgns_train_part, the restatement of ELF @0x40d6a0 with the partition filter -- to the 2e-4 of the unpartitioned
    test.  hogwild_path 1 runs the Hogwild instantiation (delta write-back, reload-on-update, atomic centre row) on the one wavefront, 9 the same
    with every node of >= HOT_THR = 15 tokens hot (never in the LDS window, negatives by atomic add): of the bucket's 2 264 pairs 67 % take the fast path
    with a hot negative, 9 % without one, 24 % the slow path, 16 % have a hot context -- asserted from the CPU classifier before the launch.  (Up to here
    the threshold was 30 on a corpus whose largest token count is 23: no node was hot and the launch never entered a hot branch.)  segments: the corpus as
    two shards of unequal length with their own walk ids (the N-rank layout), including a padded tail."""
    _bucket_case(sbm1024, d, parts, bucket, flags, hogwild_path, segments)


@pytest.mark.parametrize('d,parts,bucket,segments,fresh,local_key', [(64, 5, (3, 1), False, 3, False),          # the case above with both fresh bits (whole-walk mode)
                                                                     (128, 2, (0, 1), False, 0, False), (128, 2, (0, 1), False, 3, False),      # FULL, sliding window
                                                                     (129, 2, (0, 1), False, 0, False), (129, 2, (0, 1), False, 3, False),      # <1, 4>: the `< dg` guards
                                                                     (96, 3, (2, 0), True, 3, False),           # segment table: walk ids per shard, counts by GLOBAL id v * parts + part
                                                                     (64, 5, (3, 1), False, 0, True)])          # the locally-hot key INT32_MAX in the count buffer
def test_train_part_hot_and_fresh_rows_match_oracle(sbm1024, d, parts, bucket, segments, fresh, local_key):
    """The hot-row and fresh-row branches of the bucket kernel (sgns_win_kernel<.., PART> with DELTA, RELOAD, !ALLC) on ONE wavefront against
    oracle_sgns_train_part at 2e-4: nodes of >= 15 tokens hot as contexts (never cached, neu1e by atomic add), as negatives (atomic add of g * xc; bit 1:
    re-fetched before the dot products) and, under bit 0 or with the key INT32_MAX, as centre words (returning atomic add, no closing add).  Shares of the
    bucket's pairs by the CPU classifier at threshold 15 -- fast path with a hot negative / without / slow path, hot centre, hot context:
    5 partitions (3, 1): 67 / 9 / 24 %, 21 %, 16 %;  2 partitions (0, 1): 67 / 17 / 16 %, 17 %, 16 %;  3 partitions (2, 0), two shards: 64 / 17 / 19 %, 15 %, 15 %."""
    _bucket_case(sbm1024, d, parts, bucket, 11, 9, segments, fresh=fresh, local_key=local_key)


def test_train_part_with_one_partition_is_train(sbm1024):
    """parts == 1: the bucket is everything and gemhip_sgns_train_part is gemhip_sgns_train -- same kernel body, same draws; the two differ only in
    WHICH pairs take the exact sequential path (the bucket kernel tests a slot against the previous two slots that have a context, the plain kernel
    against the previous two slots), i.e. in the summation order of a few dot products: equal to the 2e-4 of the oracle tests."""
    n, src, dst, b = backend(sbm1024, 32)
    b.walks(1.0, 1.0, 1, 40, 5, 11, 0, 200)
    b.vocab(); b.build_unigram(); b.build_unigram_parts(1)
    P, N = b.init_tables(5)
    b.train(10, 1, 0, 0, 200, 200 * 40, 0, 5, 11 | 4)
    torch.cuda.synchronize()
    P1, N1 = P.clone(), N.clone()
    b.init_tables(5)
    nw = C.c_int64(); wl = C.c_int32(); p = C.c_void_p()
    _hip.check(b.L.gemhip_n2v_walks_ptr(b.h, C.byref(p), C.byref(nw), C.byref(wl)))
    _hip.check(b.L.gemhip_sgns_train_part(b.h, p, 200, 40, None, 0, 0, 0, 10, 0.025, 200 * 40, 0, 0, 5, 11 | 4, 0, 0, C.c_void_p(P.data_ptr()),
                                          C.c_void_p(N.data_ptr()), 32, None))
    torch.cuda.synchronize()
    for a, z in ((P, P1), (N, N1)):
        assert float((a - z).abs().max()) <= 2e-4 * float(z.abs().max()) + 1e-6
    b.close()


@pytest.mark.hogwild_stat
@pytest.mark.parametrize('parts', [1, 4])
def test_partitioned_schedule_quality_on_one_gpu(sbm1024, parts):
    """The episode schedule through the HIP backend with `parts` virtual ranks (Node2VecPartitioned.run_virtual; parts = 1 is the real world-1 run):
    every pair of TrainModel is trained exactly once and the MAP equals the sequential algorithm's.  On a 1024-node graph Hogwild itself costs a
    few percent (the launch rule bounds the open fraction of a 1024 / parts-row partition) -- hence the 8 % bar over 3 seeds."""
    n, src, dst, b = backend(sbm1024, 16)
    maps = []
    rp, col, _ = oracle.sorted_csr(n, src, dst, None)
    for seed in (1, 2, 3):
        job = multi_gpu.Node2VecPartitioned(b, multi_gpu.TorchComm(1), 0, 1, n, 10, 80, 10, 1, seed=seed, flags=9, episodes=16)
        P = (job.run(1.0, 1.0) if parts == 1 else job.run_virtual(parts)).cpu().numpy().astype(np.float64)
        if seed == 1:
            assert job.pairs_trained == len(oracle.sgns_pairs(oracle.n2v_walks(rp, col, None, None, 1.0, 1.0, 10, 80, 1, 9), 10, 0, 0, 1))
        m = node2vec(d=16, max_iter=1, walk_len=80, num_walks=10, con_size=10, ret_p=1, inout_p=1)
        maps.append(gr.evaluateStaticGraphReconstruction(sbm1024, m, P, None)[0])
    Xs, _ = oracle.n2v_train(n, src, dst, None, 16, 80, 10, 10, 1, 1.0, 1.0, 1, 9)
    MAPs = gr.evaluateStaticGraphReconstruction(sbm1024, m, Xs.astype(np.float64), None)[0]
    assert abs(np.mean(maps) - MAPs) <= 0.08 * MAPs, (maps, MAPs)
    b.close()


@pytest.mark.hogwild_stat
def test_partitioned_16k_four_virtual_ranks_match_race_free_snap():
    """SBM 16384 / d = 128 with FOUR virtual ranks (16 buckets per episode, 64 episodes): the MAP of the partitioned schedule equals the reference
    binary's race-free run (tests/golden/n2v_ref_16k.json: 0.926) within 1 % -- the N > 1 counterpart of the single-GPU test below."""
    ref = json.load(open(golden_path('n2v_ref_16k.json')))
    p = ref['params']
    g = sbm_graph(p['n'], p['edges'], p['blocks'], p['seed'])
    n, src, dst, b = backend(g, p['d'])
    job = multi_gpu.Node2VecPartitioned(b, multi_gpu.TorchComm(1), 0, 1, n, p['num_walks'], p['walk_len'], p['window'], 1, seed=3, flags=11, episodes=64)
    P = job.run_virtual(4).cpu().numpy().astype(np.float64)
    m = node2vec(d=p['d'], max_iter=1, walk_len=p['walk_len'], num_walks=p['num_walks'], con_size=p['window'], ret_p=1, inout_p=1)
    MAP = gr.evaluateStaticGraphReconstruction(g, m, P, None)[0]
    assert abs(MAP - ref['snap']['t1']['MAP']) <= 0.01 * ref['snap']['t1']['MAP'], (MAP, ref['snap'])
    b.close()


@pytest.mark.hogwild_stat
def test_sbm16k_map_matches_race_free_snap():
    """SBM 16384 nodes / 164k edges, d=128: the real binary single-threaded reaches MAP 0.926 (8 threads: 0.289,
    tests/golden/n2v_ref_16k.json, scripts/make_golden_n2v_16k.py).  The HIP path (Hogwild, auto width) must match the
    race-free value within 1 %."""
    ref = json.load(open(golden_path('n2v_ref_16k.json')))
    p = ref['params']
    g = sbm_graph(p['n'], p['edges'], p['blocks'], p['seed'])
    m = node2vec(d=p['d'], max_iter=1, walk_len=p['walk_len'], num_walks=p['num_walks'], con_size=p['window'], ret_p=1, inout_p=1, seed=3)
    Y = m.learn_embedding(graph=g, is_weighted=True, no_python=True)
    MAP = gr.evaluateStaticGraphReconstruction(g, m, Y, None)[0]
    assert abs(MAP - ref['snap']['t1']['MAP']) <= 0.01 * ref['snap']['t1']['MAP'], (MAP, ref['snap'])
    assert MAP > ref['snap']['t8']['MAP']


@pytest.mark.hogwild_stat
def test_partitioned_1m_two_virtual_ranks_inside_the_stated_n_gpu_tolerance():
    """BASELINE configs[3] at N = 2: the partitioned schedule on SBM 1M/10M with two VIRTUAL ranks (the one-GPU box; the buckets of a round touch
    disjoint rows, so running them rank after rank computes what two GPUs compute), 64 episodes, the plugin's table layout, against the sequential oracle's
    run on the same seed (tests/golden/n2v_ref_oracle_1000k_vocab_order_s4096.json, paired over its 4 096 nodes).  The schedule trains a walk's pairs in N^2
    passes spread over an episode instead of back to back, which optimises slightly BETTER than TrainModel's order (+2.8 ... +3.1 % at N = 2, 4, 8 in round 4;
    the schedule's CPU emulation without any concurrency: +0.7 ... +1.7 %): the stated N >= 2 tolerance is +4 / -1 %, asserted here."""
    import os
    path = golden_path('n2v_ref_oracle_1000k_vocab_order_s4096.json')
    if not os.path.exists(path):
        pytest.skip('no 1M oracle run in the plugin layout committed')
    ref = json.load(open(path))
    p = ref['params']
    g = sbm_graph(p['n'], p['edges'], p['blocks'], p['seed'])
    n, src, dst, b = backend(g, p['d'])
    b.vocab_order = True
    job = multi_gpu.Node2VecPartitioned(b, multi_gpu.TorchComm(1), 0, 1, n, p['num_walks'], p['walk_len'], p['window'], 1, seed=20260923, flags=p['flags'], episodes=64)
    P = job.run_virtual(2).cpu().numpy()
    nodes = np.random.RandomState(0).choice(g.n, size=len(ref['ap']), replace=False)
    ap = gr.sampled_ap_gpu(g, None, P, nodes)
    dd = ap - np.asarray(ref['ap'])
    gap, se = float(dd.mean() / ref['MAP']), float(dd.std(ddof=1) / np.sqrt(len(dd)) / ref['MAP'])
    from conftest import record_stat
    record_stat('SBM 1M/10M, partitioned schedule with 2 virtual ranks against the sequential oracle (paired, %d nodes)' % len(dd),
                '%+.2f %% (s.e. %.2f %%); kernel seconds per rank %s' % (100 * gap, 100 * se, [round(v, 2) for v in getattr(job, 'virtual_rank_seconds', [])]), '-1 ... +4 %')
    assert -0.01 <= gap <= 0.04, (gap, se)
    b.close()


def test_locally_hot_rows_reach_the_bucket_launches():
    """Round 6: the partitioned schedule builds the locally-hot key from the GATHERED corpus (gemhip_n2v_locally_hot_corpus, called by Node2VecPartitioned and by
    gemhip_n2v_train_multi): on an SBM with a dozen isolated edges appended exactly their ends qualify, a Hogwild bucket launch then carries the hot-row
    machinery with the threshold INT32_MAX (only those nodes), and the deterministic schedule is untouched (equal to the run with the rule off, bit for bit)."""
    from test_n2v_gpu import _graph_with_isolated_edges
    n, src, dst = _graph_with_isolated_edges(n_core=16384, iso_pairs=12)
    row_ptr, col, ww = to_csr(n, src, dst, None)
    res = {}
    for rule in (8, 0):
        b = multi_gpu.HipBackendN2V(n, row_ptr, col, ww, 32)
        job = multi_gpu.Node2VecPartitioned(b, multi_gpu.TorchComm(1), 0, 1, n, 2, 40, 5, 1, seed=3, flags=9, episodes=2)
        if rule == 0:
            b.locally_hot = lambda corpus: 0                 # rule off: the driver's hook does nothing
        P = job.run_virtual(2)
        k, wv, hot, fr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _hip.check(b.L.gemhip_sgns_last_launch(b.h, C.byref(k), C.byref(wv), C.byref(hot), C.byref(fr)))
        res[rule] = (hot.value, wv.value, bool(torch.isfinite(P).all()))
        b.close()
    assert res[8][0] == np.iinfo(np.int32).max and res[8][1] > 1 and res[8][2]
    assert res[0][0] == 0 and res[0][2]
    # the count itself, and the deterministic schedule with and without the rule
    b = multi_gpu.HipBackendN2V(n, row_ptr, col, ww, 32)
    job = multi_gpu.Node2VecPartitioned(b, multi_gpu.TorchComm(1), 0, 1, n, 2, 40, 5, 1, seed=3, flags=9 | 4, episodes=2)
    Pa = job.run_virtual(2).cpu().numpy()
    corpus = b.gather_corpus(multi_gpu.TorchComm(1), job.shard_rows, 1)
    assert b.locally_hot(corpus) == 12 * 2 + 3
    b.locally_hot = lambda corpus: 0
    Pb = multi_gpu.Node2VecPartitioned(b, multi_gpu.TorchComm(1), 0, 1, n, 2, 40, 5, 1, seed=3, flags=9 | 4, episodes=2).run_virtual(2).cpu().numpy()
    assert np.array_equal(Pa, Pb)
    b.close()


@pytest.mark.parametrize('d', [16, 130])
def test_one_handle_serves_both_table_sets_and_both_layouts(d):
    """A handle holds two sets of unigram tables -- the single one of gemhip_sgns_train and the per-partition one of gemhip_sgns_train_part -- and
    either in two layouts, each with a slot table built on first use.  Deterministic launches on one wavefront, 2 walks of 13 tokens per node, window 3:
    (a) building the two-partition tables and training a bucket leaves the single table's launches as they were: the same start tables give the
        same result, bit for bit, without a rebuild;
    (b) after a launch in the binary's layout, a build in the node-id layout trains exactly what a fresh handle trains: the second launch does not
        draw from the first layout's slot table."""
    from test_oracle_n2v import small_graph
    n, src, dst, _ = small_graph(False, seed=3, n=200, m=3000)
    row_ptr, col, _ = oracle.sorted_csr(n, src, dst, None)
    L, l, window, seed = _hip.lib(), 13, 3, 3
    rs = np.random.RandomState(d)
    P0, N0 = (0.05 * rs.randn(n, d)).astype(np.float32), (0.05 * rs.randn(n, d)).astype(np.float32)

    def handle():
        h, m = C.c_void_p(), C.c_int64()
        _hip.check(L.gemhip_n2v_create(n, len(col), _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), None, C.byref(h)))
        _hip.check(L.gemhip_n2v_start_nodes(h, C.byref(m)))
        _hip.check(L.gemhip_n2v_walks(h, 1.0, 1.0, 2, l, seed, 11, 0, 2 * m.value, None))
        _hip.check(L.gemhip_n2v_vocab(h, None))
        _hip.check(L.gemhip_sgns_init(h, d, seed, None, None))
        return h, 2 * m.value

    def train(h, nwalks, flags):
        """one epoch of gemhip_sgns_train from the fixed start tables -> (SynPos, SynNeg)"""
        _hip.check(L.gemhip_sgns_set_tables(h, _hip.ptr(P0, C.c_float), _hip.ptr(N0, C.c_float)))
        _hip.check(L.gemhip_sgns_train(h, window, 5, 0.025, 1, 0, 0, nwalks, nwalks * l, 0, seed, flags | 4, None))
        P, N = np.empty_like(P0), np.empty_like(N0)
        _hip.check(L.gemhip_sgns_get_tables(h, _hip.ptr(P, C.c_float), _hip.ptr(N, C.c_float)))
        return P, N

    h, nwalks = handle()
    _hip.check(L.gemhip_n2v_build_unigram(h, None, None, None))
    T = train(h, nwalks, 11)
    assert not np.array_equal(T[0], P0) and not np.array_equal(T[1], N0)
    # (a) the same handle: two-partition tables, one bucket, then the single table again
    _hip.check(L.gemhip_n2v_build_unigram_parts(h, 2, None, None))
    Pp = torch.from_numpy(P0[0::2].copy()).cuda(); Np = torch.from_numpy(N0[1::2].copy()).cuda()
    walks, nw, wl = C.c_void_p(), C.c_int64(), C.c_int32()
    _hip.check(L.gemhip_n2v_walks_ptr(h, C.byref(walks), C.byref(nw), C.byref(wl)))
    _hip.check(L.gemhip_sgns_train_part(h, walks, nwalks, l, None, 0, 0, 0, window, 0.025, nwalks * l, 0, 0, seed, 11 | 4, 0, 1, C.c_void_p(Pp.data_ptr()),
                                          C.c_void_p(Np.data_ptr()), d, None))
    torch.cuda.synchronize()
    assert not np.array_equal(Pp.cpu().numpy(), P0[0::2])                 # (the bucket did train)
    again = train(h, nwalks, 11)
    assert np.array_equal(again[0], T[0]) and np.array_equal(again[1], T[1])
    _hip.check(L.gemhip_n2v_destroy(h))
    # (b) one handle: the binary's layout, a launch, then the node-id layout
    h, nwalks = handle()
    _hip.check(L.gemhip_n2v_build_unigram_vocab_order(h, 11, None, None, None, None))
    V = train(h, nwalks, 27)
    assert not np.array_equal(V[1], T[1])                                 # (the layouts are different tables: different negatives)
    _hip.check(L.gemhip_n2v_build_unigram(h, None, None, None))
    again = train(h, nwalks, 11)
    assert np.array_equal(again[0], T[0]) and np.array_equal(again[1], T[1])
    _hip.check(L.gemhip_n2v_destroy(h))
