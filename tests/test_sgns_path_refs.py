"""CPU tests: tests/sgns_path_refs.py -- the branch classifier the SGNS hot-row GPU tests assert their coverage with -- tied to the oracle: it forms the
pairs oracle_sgns_pairs forms and draws the targets oracle_sgns_train / oracle_sgns_train_part update, so the shares it reports are shares of what is
trained.  Also pins the two corpora of tests/test_sgns_hot_paths_gpu.py: the class shares the floors are asserted on are computed here without a device."""
import numpy as np
import pytest

import oracle
import sgns_path_refs as spr
from gem_amd.graph import edge_arrays

SNAP = 11


def corpus(G, nwalks, l, seed, lo=0):
    n, src, dst, w, _ = edge_arrays(G)
    row_ptr, col, _ = oracle.sorted_csr(n, src, dst, w)
    walks = oracle.n2v_walks(row_ptr, col, None, None, 1.0, 1.0, 1, l, seed, SNAP, lo, lo + nwalks)
    counts = oracle.n2v_vocab(n, walks)
    return n, walks, counts


@pytest.mark.parametrize('window,epoch,wid0', [(5, 0, 0), (3, 2, 7), (10, 0, 1 << 33)])
def test_pairs_are_train_models_pairs(sbm1024, window, epoch, wid0):
    n, walks, counts = corpus(sbm1024, 12, 20, 5)
    walks = walks.copy()
    walks[3, 15:] = -1; walks[7, 4] = -1                      # a padded tail and a hole: TrainModel skips both as centre and as context
    UT, KT = oracle.unigram_build(counts)
    cls = spr.pair_classes(walks, window, 9, epoch, UT, KT, n, counts, 4, walk_id_offset=wid0)
    want = oracle.sgns_pairs(walks, window, epoch, wid0, 9)
    assert len(want) > 500
    assert np.array_equal(np.stack([cls['ctx'], cls['word']], 1), want)
    # the hole makes the valid contexts of its neighbours' centres non-contiguous: the kernel sends every pair of such a centre down the exact path
    around = (cls['word'] == walks[7, 3]) | (cls['word'] == walks[7, 5])
    assert cls['special'][around].any()


@pytest.mark.parametrize('flags', [SNAP, 9])
def test_targets_are_the_rows_train_model_updates(sbm1024, flags):
    n, walks, counts = corpus(sbm1024, 10, 20, 5)
    UT, KT = oracle.unigram_build(counts)
    cls = spr.pair_classes(walks, 5, 5, 0, UT, KT, n, counts, 4, flags=flags)
    P, N = oracle.sgns_init(n, 8, 5)
    assert not N.any()
    oracle.sgns_train(walks, 5, 0.025, 1, 0, walks.size, 0, 0, UT, KT, 5, flags, P, N)
    got = set(np.flatnonzero(np.abs(N).max(1) > 0).tolist())
    assert got == spr.updated_neg_rows(cls) and len(got) > 100


@pytest.mark.parametrize('parts,bucket,wids', [(2, (0, 1), None), (5, (3, 1), None), (3, (2, 2), 1000)])
def test_bucket_targets_are_the_rows_train_part_updates(sbm1024, parts, bucket, wids):
    n, walks, counts = corpus(sbm1024, 40, 20, 3)
    gi, gj = bucket
    UT, KT, off = oracle.unigram_build_parts(counts, parts)
    UTp, KTp = UT[off[gj]:off[gj + 1]], KT[off[gj]:off[gj + 1]]
    ids = None if wids is None else np.arange(len(walks), dtype=np.int64)[::-1] + wids
    cls = spr.pair_classes(walks, 5, 3, 0, UTp, KTp, len(UTp), counts, 4, wids=ids, bucket=(parts, gi, gj))
    assert (cls['ctx'] % parts == gi).all() and (cls['word'] % parts == gj).all() and (cls['targets'] % parts == gj).all()
    P, N = oracle.sgns_init(n, 8, 3)
    npairs = oracle.sgns_train_part(walks, ids, 5, 0.025, walks.size, 0, 0, parts, gi, gj, UTp, KTp, 3, SNAP, P, N)
    assert npairs == len(cls['ctx']) > 50
    # the bucket's pairs are the unrestricted pairs filtered by partition, in order
    allp = oracle.sgns_pairs(walks, 5, 0, 0, 3) if wids is None else None
    if allp is not None:
        keep = (allp[:, 0] % parts == gi) & (allp[:, 1] % parts == gj)
        assert np.array_equal(np.stack([cls['ctx'], cls['word']], 1), allp[keep])
    got = set(np.flatnonzero(np.abs(N).max(1) > 0).tolist())
    assert got == spr.updated_neg_rows(cls)


def test_special_rule_on_a_hand_made_table():
    """One walk over three nodes with a two-entry-heavy table: nearly every pair repeats a target (special); the classes follow key / thr / fresh."""
    walks = np.array([[0, 1, 2, 0, 1, 2, 0, 1]], np.int32)
    counts = np.array([3, 3, 2], np.int32)
    UT, KT = oracle.unigram_build(counts)
    cls = spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, counts, 3, fresh=0)
    assert cls['special'].all()                                    # five draws from three nodes: a target is always drawn twice
    assert np.array_equal(cls['hot_ctx'], cls['ctx'] < 2) and not cls['hot_word'].any()
    assert np.array_equal(spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, counts, 3, fresh=1)['hot_word'], cls['word'] < 2)
    key = np.array([spr.INT32_MAX, 3, 2], np.int32)
    loc = spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, key, spr.INT32_MAX)
    assert np.array_equal(loc['hot_word'], loc['word'] == 0) and np.array_equal(loc['hot_ctx'], loc['ctx'] == 0)
    # bit 2: a target is hot from neg_thr on, whatever thr says
    assert not spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, counts, spr.INT32_MAX, fresh=0)['hot_neg'].any()
    assert spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, counts, spr.INT32_MAX, neg_thr=0, fresh=4)['hot_neg'].all()
    # radius 1 of window 2: a context two positions away is fetched per pair unless its node also sits next to the centre -- in this period-3 walk it
    # always does, except at the two ends of the walk, where the centre has one neighbour only
    r1 = spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, counts, 100, radius=1)
    assert set(r1['word'][r1['beyond']].tolist()) <= {int(walks[0, 0]), int(walks[0, -1])}
    assert not spr.pair_classes(walks, 2, 1, 0, UT, KT, 3, counts, 100, radius=2)['beyond'].any()


@pytest.mark.parametrize('nwalks,l,window,thr,want', [(64, 20, 5, 4, (0.45, 0.39, 0.16, 0.13, 0.13)), (96, 24, 10, 5, (0.69, 0.14, 0.17, 0.20, None))])
def test_the_gpu_corpora_reach_every_class(sbm1024, nwalks, l, window, thr, want):
    """The two corpora of tests/test_sgns_hot_paths_gpu.py (SBM-1024, seed 5, the first 64 walks of 20 tokens at window 5 / 96 of 24 at window 10): the
    shares of the pairs that take the fast path with a hot negative, the fast path without one, the slow path, and that have a hot centre word / a hot
    context, each above the 5 % floor -- and where they were measured when the cases were chosen (within 0.02)."""
    n, walks, counts = corpus(sbm1024, nwalks, l, 5)
    UT, KT = oracle.unigram_build(counts)
    cls = spr.pair_classes(walks, window, 5, 0, UT, KT, n, counts, thr, fresh=3)
    s = spr.assert_floors(cls, ('fast_hot', 'fast_cold', 'slow', 'hot_word', 'hot_ctx'))
    print(s, int((counts >= thr).sum()), int((counts > 0).sum()))
    for k, w in zip(('fast_hot', 'fast_cold', 'slow', 'hot_word', 'hot_ctx'), want):
        if w is not None:
            assert abs(s[k] - w) <= 0.02, (k, s)
    assert s['slow_hot'] >= 0.25 * s['slow']
    r2 = spr.shares(spr.pair_classes(walks, window, 5, 0, UT, KT, n, counts, thr, fresh=3, radius=2))
    assert r2['beyond'] >= spr.FLOOR
