"""GPU tests: the hot-row and fresh-row branches of the shipped Hogwild instantiation of sgns_win_kernel (<.., DELTA, RELOAD, !ALLC>: gem_amd/csrc/sgns.hpp)
on ONE wavefront against oracle.sgns_train.  On one wavefront every one of those branches is still TrainModel's arithmetic -- a returning atomic add returns
the register copy, a re-fetched row is the row the sequential algorithm reads, an atomic add of g * xc is the store it replaces -- so the bar is the one of
every deterministic SGNS test, max|got - want| <= 2e-4 max|want| + 1e-6.  Every case first proves on the CPU (tests/sgns_path_refs.py, tied to the oracle by
tests/test_sgns_path_refs.py) that its corpus REACHES the branches it is there for: at least 5 % of the pairs in each class, and asserts the launch it got
(gemhip_sgns_last_launch): the Hogwild window kernel, one wavefront, the threshold and the fresh bits asked for."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import sgns_path_refs as spr
from gem_amd import _hip, multi_gpu
from gem_amd.graph import edge_arrays, to_csr
from test_n2v_gpu import Dev

pytestmark = pytest.mark.gpu
SNAP, SEED, INT32_MAX = 11, 5, spr.INT32_MAX
# SBM-1024, p = q = 1, one round, seed 5: (walks, tokens per walk, window, hot threshold).  'A': 6 854 pairs, 40 hot nodes of the 719 that occur;
# 'B': 2 x window x 5 = 100 > 64 negative samples per centre, two per lane
CORPORA = {'A': (64, 20, 5, 4), 'B': (96, 24, 10, 5)}
_cache = {}


def _memo(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _bar(got, want):
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print('max|got - want| = %.3e, bar %.3e (max|want| = %.3e)' % (err, 2e-4 * scale + 1e-6, scale))
    assert err <= 2e-4 * scale + 1e-6, (err, scale)


def _oracle_tables(name, d, walks, UT, KT, n):
    """oracle.sgns_train on the corpus from oracle.sgns_init: computed once per (corpus, d), shared and never written to"""
    def make():
        P, N = oracle.sgns_init(n, d, SEED)
        oracle.sgns_train(walks, CORPORA[name][2], 0.025, 1, 0, walks.size, 0, 0, UT, KT, SEED, SNAP, P, N)
        P.setflags(write=False); N.setflags(write=False)
        return P, N
    return _memo(('oracle', name, d), make)


def _classes(name, walks, UT, KT, n, key, thr, neg_thr, fresh, radius, tag=''):
    return _memo(('cls', name, thr, neg_thr, fresh, radius, tag),
                 lambda: spr.pair_classes(walks, CORPORA[name][2], SEED, 0, UT, KT, n, key, thr, neg_thr=neg_thr, fresh=fresh, radius=radius, flags=SNAP))


def _last_launch(L, h):
    k, wv, hot, fr = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    _hip.check(L.gemhip_sgns_last_launch(h, C.byref(k), C.byref(wv), C.byref(hot), C.byref(fr)))
    return k.value, wv.value, hot.value, fr.value


#   d    corpus radius fresh neg_count thr (None: the corpus's)      instantiation <VEC, NV, FULL>
CASES = [(128, 'A', -1, 0, 0, None), (128, 'A', -1, 1, 0, None), (128, 'A', -1, 2, 0, None), (128, 'A', -1, 3, 0, None),     # <2, 1, FULL>
         (128, 'B', -1, 0, 0, None), (128, 'B', -1, 3, 0, None),                   # two negative samples per lane
         (128, 'A', 2, 0, 0, None), (128, 'A', 2, 3, 0, None),                     # contexts beyond the radius take their atomic add next to the hot ones
         (96, 'A', -1, 0, 0, None), (96, 'A', -1, 3, 0, None),                     # <2, 1, !FULL>: the `< dg` guard on every atomic
         (33, 'A', -1, 3, 0, None),                                                # <1, 1, !FULL>
         (129, 'A', -1, 1, 0, None),                                               # <1, 4, !FULL>
         (256, 'A', 5, 3, 0, None),                                                # <2, 2, FULL>
         (128, 'A', -1, 4, 0, INT32_MAX),                                          # bit 2 alone: nothing hot by count, EVERY negative row updated by atomic add
         (128, 'A', -1, 4, 4, INT32_MAX),                                          # bit 2 with a count that splits the negatives: >= 4 tokens atomic add, else reload + store
         (128, 'A', 2, 7, 2, None)]                                                # everything at once


@pytest.mark.parametrize('d,corpus,radius,fresh,neg_count,thr', CASES)
def test_hot_and_fresh_rows_on_one_wavefront_match_oracle(sbm1024, monkeypatch, d, corpus, radius, fresh, neg_count, thr):
    """gemhip_sgns_train, flags | 4, with the Hogwild code path forced (gemhip_sgns_set_window_cache(h, radius, 1)), hot rows from `thr` tokens on and the
    fresh bits: SynPos and SynNeg against oracle.sgns_train at 2e-4.  Class shares ('A', thr 4, helper's count): fast path with a hot negative 45 %,
    without 39 %, slow path 16 % (half with a hot target), hot centre word 13 % (bit 0), hot context 13 %, radius 2 of window 5: 32 % beyond the radius;
    'B' (thr 5): 69 / 14 / 17 %, hot centre 20 %, hot context 20 %.  Bit 2 with neg_count 0 or 2: EVERY fast-path pair has a hot negative (84 %; under
    RndUnigramInt's quirk only alias targets are drawn, and those have at least 2 tokens), so the cold fast path is asserted to be empty there instead;
    neg_count 4 splits the negatives like the threshold does (45 / 39 %) with no hot context or centre."""
    nwalks, l, window, thr0 = CORPORA[corpus]
    thr = thr0 if thr is None else thr
    monkeypatch.setenv('GEMHIP_SGNS_NEG_COUNT', str(neg_count))                    # (read in gemhip_n2v_create: there is no setter)
    n, src, dst, w, _ = edge_arrays(sbm1024)
    dev = Dev(n, src, dst, w)
    walks = dev.walks(1.0, 1.0, 1, l, SEED, SNAP, 0, nwalks)
    counts, UT, KT = dev.unigram()
    # coverage first: the corpus reaches the branches this case is there for
    need = ['fast_hot', 'slow']
    cold = not (fresh & 4) or neg_count > 2
    if cold:
        need.append('fast_cold')
    if thr < INT32_MAX:
        need.append('hot_ctx')
        if fresh & 1:
            need.append('hot_word')
    if 0 <= radius < window:
        need.append('beyond')
    cls = _classes(corpus, walks, UT, KT, n, counts, thr, neg_count, fresh, radius)
    s = spr.assert_floors(cls, need)
    print({k: round(float(v), 4) for k, v in s.items()})
    if thr == INT32_MAX:
        assert s['hot_ctx'] == 0 and s['hot_word'] == 0
    if not cold:
        assert s['fast_cold'] == 0
    assert s['slow_hot'] >= spr.FLOOR
    L = dev.L
    _hip.check(L.gemhip_sgns_set_window_cache(dev.h, radius, 1))
    _hip.check(L.gemhip_sgns_set_hot_rows(dev.h, thr))
    _hip.check(L.gemhip_sgns_set_fresh(dev.h, fresh))
    P, N = dev.sgns(d, window, 1, SEED, SNAP | 4)
    assert _last_launch(L, dev.h) == (2, 1, thr, fresh)
    pairs = C.c_int64(); _hip.check(L.gemhip_sgns_pairs(dev.h, C.byref(pairs), 0))
    assert pairs.value == s['pairs']
    Po, No = _oracle_tables(corpus, d, walks, UT, KT, n)
    _bar(N, No); _bar(P, Po)
    dev.close()


@pytest.mark.parametrize('d', [128, 96])
def test_locally_hot_key_on_one_wavefront_matches_oracle(sbm1024, d):
    """The DEFAULT path of a locally hot node (hot key INT32_MAX, no fresh bit): kept out of the LDS window, updated as a negative by atomic add, and as a
    centre word through the returning atomic add of pos_update with the closing add skipped.  A Hogwild launch hands the kernel n2v.hip's hot key only when
    it has more than one wavefront; here the key is written into the count buffer the handle was bound to (gemhip_n2v_bind_counts) after the unigram table
    was built from the real counts: INT32_MAX for the nodes of >= 4 tokens, the count elsewhere, threshold INT32_MAX.  Same classes as corpus 'A' at
    threshold 4 with bit 0: 45 / 39 / 16 %, hot centre 13 %, hot context 13 %."""
    nwalks, l, window, thr0 = CORPORA['A']
    n, src, dst, w, _ = edge_arrays(sbm1024)
    row_ptr, col, ww = to_csr(n, src, dst, w)
    b = multi_gpu.HipBackendN2V(n, row_ptr, col, ww, d)
    b.walks(1.0, 1.0, 1, l, SEED, SNAP, 0, nwalks)
    walks = np.empty((nwalks, l), np.int32)
    _hip.check(b.L.gemhip_n2v_get_walks(b.h, _hip.ptr(walks, C.c_int32)))
    b.vocab(); b.build_unigram()
    counts = b.counts.cpu().numpy().copy()
    UT, KT = oracle.unigram_build(counts)
    key = np.where(counts >= thr0, INT32_MAX, counts).astype(np.int32)
    cls = _classes('A', walks, UT, KT, n, key, INT32_MAX, 0, 0, -1, tag='local')
    s = spr.assert_floors(cls, ('fast_hot', 'fast_cold', 'slow', 'hot_word', 'hot_ctx'))
    print({k: round(float(v), 4) for k, v in s.items()})
    assert np.array_equal(cls['hot_word'], key[cls['word']] == INT32_MAX)
    b.counts.copy_(torch.from_numpy(key))
    torch.cuda.synchronize()
    _hip.check(b.L.gemhip_sgns_set_window_cache(b.h, -1, 1))
    _hip.check(b.L.gemhip_sgns_set_hot_rows(b.h, INT32_MAX))
    _hip.check(b.L.gemhip_sgns_set_fresh(b.h, 0))
    P, N = b.init_tables(SEED)
    b.train(window, 1, 0, 0, nwalks, nwalks * l, 0, SEED, SNAP | 4)
    torch.cuda.synchronize()
    assert _last_launch(b.L, b.h) == (2, 1, INT32_MAX, 0)
    assert b.pairs() == s['pairs']
    Po, No = _oracle_tables('A', d, walks, UT, KT, n)
    _bar(N.cpu().numpy(), No); _bar(P.cpu().numpy(), Po)
    b.close()
