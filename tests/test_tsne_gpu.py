"""GPU: gem_amd/csrc/tsne.hip stage by stage against the host restatements of tests/tsne_refs.py and the sklearn fixtures of
scripts/make_golden_tsne.py.  The map from test to reference, the fixtures and every measured tolerance: tests/README_tsne.md.

Shapes: n = 34 (k = n - 1, one partial tile holds every row), n = 300 with d = 128, n = 1061 with d = 33 (prime and odd: ragged row blocks,
ragged j-slices, an unaligned row stride), k = 16 and k = 301."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import tsne_refs as R
from gem_amd import _hip
from gem_amd.evaluation import tsne

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def golden():
    g = np.load(os.path.join(R.GOLDEN, 'tsne_affinities_ref.npz'))
    return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def inputs(tag):
    return {'normal': R.normal_input, 'karate': R.karate_input, 'prime': R.prime_input}[tag]()


@functools.lru_cache(maxsize=None)
def true_distances(tag):
    D = R.squared_distances(inputs(tag))
    D.setflags(write=False)
    return D


def knn_with_stride(X, k, ld):
    """gemhip_tsne_knn on X laid out with row stride ld >= d (the padding holds NaN: it must never be read as data)."""
    n, d = X.shape
    buf = np.full((n, ld), np.nan, np.float32)
    buf[:, :d] = X
    ids = np.full((n, k), -7, np.int32); dist = np.full((n, k), -7, np.float32)
    _hip.check(_hip.lib().gemhip_tsne_knn(n, d, ld, _hip.ptr(buf, C.c_float), k, _hip.ptr(ids, C.c_int32), _hip.ptr(dist, C.c_float)))
    return ids, dist


# ------------------------------------------------------------------ 1. kNN
@pytest.mark.parametrize('tag,k,pad', [('karate', 33, 0), ('normal', 91, 0), ('normal', 91, 3), ('prime', 16, 0), ('prime', 301, 0), ('prime', 91, 4)])
def test_knn_against_fp64_brute_force(tag, k, pad):
    X = inputs(tag); D = true_distances(tag)
    n, d = X.shape
    ids, dist = knn_with_stride(X, k, d + pad)
    bound = R.knn_bound(X)
    rows = np.arange(n)[:, None]
    assert ids.min() >= 0 and ids.max() < n and not np.any(ids == rows)
    assert all(len(set(r)) == k for r in ids.tolist())
    asc = (dist[:, 1:] > dist[:, :-1]) | ((dist[:, 1:] == dist[:, :-1]) & (ids[:, 1:] > ids[:, :-1]))
    assert asc.all()
    true_of_ids = D[rows, ids]
    err = np.abs(dist.astype(np.float64) - true_of_ids).max()
    ref_ids, ref_d = R.sorted_knn(D, k)
    excess = (true_of_ids - ref_d[:, -1:]).max()
    print('kNN %s k=%d ld=%d: bound %.3e, returned-distance error %.3e, excess over the true k-th distance %.3e' % (tag, k, d + pad, bound, err, excess))
    assert err <= bound
    assert excess <= 2.0 * bound
    if tag == 'normal':
        assert np.array_equal(np.sort(ids, axis=1), np.sort(ref_ids, axis=1))
        assert np.array_equal(ref_ids, golden()['normal_id'])


# ------------------------------------------------------------------ 2. affinities
@pytest.mark.parametrize('tag', ['normal', 'karate'])
def test_affinities_against_sklearn(tag):
    dist = golden()[tag + '_dist']; want = golden()[tag + '_P']
    got = tsne.conditional_affinities(dist, R.PERPLEXITY)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.abs(got.sum(axis=1, dtype=np.float64) - 1.0).max() <= 1e-6
    yard = np.abs(R.binary_search_perplexity(dist, R.PERPLEXITY, np.float32).astype(np.float64) - want).max()
    dev = np.abs(got.astype(np.float64) - want).max()
    print('affinities %s: fp32 restatement deviates %.3e from sklearn, the device %.3e' % (tag, yard, dev))
    assert yard > 0
    assert dev <= 4.0 * yard


def test_affinities_other_widths():
    """k = 16 and k = 301 (one lane group partly idle; five entries per lane) against the fp64 restatement, which equals sklearn's to 1e-15 on the
    fixture: a float32 rounding of a value <= 1 is the whole allowance."""
    D = true_distances('prime')
    for k, perplexity in ((16, 5.0), (301, 100.0)):
        dist = R.sorted_knn(D, k)[1].astype(np.float32)
        got = tsne.conditional_affinities(dist, perplexity)
        want = R.binary_search_perplexity(dist, perplexity)
        assert np.abs(got.astype(np.float64) - want).max() <= EPS32
        assert np.abs(got.sum(axis=1, dtype=np.float64) - 1.0).max() <= 1e-6


# ------------------------------------------------------------------ 3. gradient, KL, Z with the caller's P
@functools.lru_cache(maxsize=None)
def normal_problem():
    ids = golden()['normal_id']; p = golden()['normal_P'].astype(np.float32)
    return ids, p, R.dense_joint(len(ids), ids, p)


def spread_embedding(n, scale, seed=1):
    return (scale * np.random.RandomState(seed).standard_normal((n, 2))).astype(np.float32)


@pytest.mark.parametrize('which', ['init', 'spread'])
@pytest.mark.parametrize('exaggeration', [1.0, 12.0])
def test_gradient_kl_z_with_the_callers_affinities(which, exaggeration):
    X = inputs('normal')
    ids, p, P = normal_problem()
    Y = tsne.pca_init(X) if which == 'init' else spread_embedding(len(X), 30.0)
    # a handle on OTHER affinities (perplexity 5 -> k = 16 would not match): same perplexity, then replaced by the caller's arrays, rows reversed
    with tsne.TsneHandle(X, R.PERPLEXITY) as h:
        h.set_affinities(ids[:, ::-1], p[:, ::-1])
        h.set_embedding(Y)
        g, kl, Z = h.gradient(exaggeration)
    want, want_kl, want_Z = R.gradient(P, Y, exaggeration)
    yard32 = R.gradient(P, Y, exaggeration, np.float32, np.random.RandomState(0).permutation(len(X)))[0]
    scale = np.abs(want).max()
    yard = np.abs(yard32 - want).max() / scale
    dev = np.abs(g - want).max() / scale
    print('gradient %s x%g: shuffled fp32 restatement deviates %.3e of |grad|inf, the device %.3e; Z rel %.3e, KL rel %.3e'
          % (which, exaggeration, yard, dev, abs(Z - want_Z) / want_Z, abs(kl - want_kl) / want_kl))
    assert dev <= 4.0 * yard
    assert abs(Z - want_Z) <= 1e-6 * want_Z
    assert abs(kl - want_kl) <= 1e-6 * want_kl


def test_gradient_on_ragged_slices_and_the_handles_own_affinities():
    """n = 1061: three row blocks and five j-slices, the last of 37 columns.  P is the handle's own (kNN + affinities + transpose on the device),
    rebuilt on the host from the same stages' outputs."""
    X = inputs('prime')
    n = len(X)
    ids, dist = tsne.knn(X, 91)
    p = tsne.conditional_affinities(dist, R.PERPLEXITY)
    P = R.dense_joint(n, ids, p)
    Y = spread_embedding(n, 5.0, seed=2)
    with tsne.TsneHandle(X, R.PERPLEXITY) as h:
        assert (h.k, h.n_slices) == (91, 5)
        h.set_embedding(Y)
        g, kl, Z = h.gradient(1.0)
    want, want_kl, want_Z = R.gradient(P, Y, 1.0)
    yard32 = R.gradient(P, Y, 1.0, np.float32, np.random.RandomState(0).permutation(n))[0]
    scale = np.abs(want).max()
    yard = np.abs(yard32 - want).max() / scale
    dev = np.abs(g - want).max() / scale
    print('gradient n=1061: yardstick %.3e, device %.3e; Z rel %.3e, KL rel %.3e' % (yard, dev, abs(Z - want_Z) / want_Z, abs(kl - want_kl) / want_kl))
    assert dev <= 4.0 * yard
    assert abs(Z - want_Z) <= 1e-6 * want_Z
    assert abs(kl - want_kl) <= 1e-6 * want_kl


# ------------------------------------------------------------------ 4. update rule
UPDATE_LR = 12.5          # n = 300: at sklearn's floor of 50 the fp32 and the fp64 restatement are 0.6 max|Y| apart after 30 steps (README_tsne.md)


def test_update_rule_thirty_steps_of_early_exaggeration():
    X = inputs('normal')
    ids, p, P = normal_problem()
    Y0 = tsne.pca_init(X)
    with tsne.TsneHandle(X, R.PERPLEXITY) as h:
        h.set_affinities(ids, p)
        h.set_embedding(Y0)
        h.run(30, 12.0, 0.5, UPDATE_LR)
        got = h.get_embedding()
    want = R.gradient_descent(P, Y0, 30, 12.0, 0.5, UPDATE_LR)[0]
    yard32 = R.gradient_descent(P, Y0, 30, 12.0, 0.5, UPDATE_LR, np.float32)[0]
    scale = np.abs(want).max()
    yard = np.abs(yard32 - want).max() / scale
    dev = np.abs(got - want).max() / scale
    print('update rule, 30 steps: fp32 restatement deviates %.3e of max|Y|, the device %.3e (max|Y| %.3e)' % (yard, dev, scale))
    assert scale > 10 * np.abs(Y0).max()                  # the steps moved the points: gains and momentum were at work
    assert dev <= 4.0 * yard


def test_arguments_of_a_second_call_take_effect_and_state_carries_over():
    """Across sklearn's switch at iteration 250, in two calls (245 + 10).  (a) The optimiser's state carries over a call boundary: 245 + 10 steps
    at fixed arguments are the bytes of one call of 255, and 245 + 10 with the switch share the 245-step prefix with it.  (b) The second call's
    exaggeration and momentum are the ones used: the switched run ends elsewhere.  After 245 steps a float32 and a float64 trajectory have long
    parted, so the QUANTITATIVE form of (b) is taken where they have not: 20 steps at (12, 0.5) then 10 at (1, 0.8) against the fp64
    restatement making the same switch, with the yardstick of the 30-step test -- and far from the restatement that does not switch."""
    X = inputs('normal')
    ids, p, P = normal_problem()
    Y0 = tsne.pca_init(X)

    def device(calls):
        with tsne.TsneHandle(X, R.PERPLEXITY) as h:
            h.set_affinities(ids, p)
            h.set_embedding(Y0)
            out = []
            for n_iter, ex, mom in calls:
                h.run(n_iter, ex, mom, UPDATE_LR)
                out.append(h.get_embedding())
        return out

    one = device([(255, 12.0, 0.5)])[0]
    two = device([(245, 12.0, 0.5), (10, 12.0, 0.5)])
    assert np.array_equal(two[1], one)
    switched = device([(245, 12.0, 0.5), (10, 1.0, 0.8)])
    assert np.array_equal(switched[0], two[0])            # the common prefix
    assert not np.array_equal(switched[1], one)
    got = device([(20, 12.0, 0.5), (10, 1.0, 0.8)])[1]

    def restated(dtype, second):
        pre, state = R.gradient_descent(P, Y0, 20, 12.0, 0.5, UPDATE_LR, dtype)
        return R.gradient_descent(P, pre, 10, second[0], second[1], UPDATE_LR, dtype, state=state)[0]

    want = restated(np.float64, (1.0, 0.8)); yard32 = restated(np.float32, (1.0, 0.8)); unswitched = restated(np.float64, (12.0, 0.5))
    scale = np.abs(want).max()
    yard = np.abs(yard32 - want).max() / scale
    dev = np.abs(got - want).max() / scale
    apart = np.abs(unswitched - want).max() / scale
    print('20 + 10 steps with the switch: fp32 restatement deviates %.3e of max|Y|, the device %.3e; the restatement without the switch is %.3e away'
          % (yard, dev, apart))
    assert apart > 100 * 4.0 * yard                       # the check can tell the two apart
    assert dev <= 4.0 * yard


# ------------------------------------------------------------------ 5. determinism
def test_two_runs_are_bit_identical_and_reduce_tsne_is_the_direct_call():
    from gem.evaluation import visualize_embedding as viz
    X = inputs('prime')
    Y1, info1 = tsne.tsne_2d(X)
    Y2, info2 = tsne.tsne_2d(X)
    assert Y1.dtype == np.float64 and Y1.shape == (len(X), 2) and np.isfinite(Y1).all()
    assert np.array_equal(Y1, Y2) and info1['kl_divergence'] == info2['kl_divergence']
    assert info1['n_iter'] == 1000 and info1['k'] == 91
    assert np.array_equal(viz.reduce_to_2d(X, reduce='tsne'), Y1)
    for key in ('knn_ms', 'affinity_ms', 'transpose_ms', 'iterations_ms'):
        assert info1[key] > 0


# ------------------------------------------------------------------ 6. end to end
def test_end_to_end_inside_sklearns_seed_to_seed_spread():
    from conftest import record_stat
    ref = json.load(open(os.path.join(R.GOLDEN, 'tsne_sbm1024_ref.json')))['runs']
    kls = [r['dense_kl'] for r in ref]; tws = [r['trustworthiness'] for r in ref]
    kl_bar = max(kls) + (max(kls) - min(kls)); tw_bar = min(tws) - (max(tws) - min(tws))
    X = R.sbm_input()
    Y, info = tsne.tsne_2d(X)
    kl = R.dense_kl(R.dense_p_of_input(X), Y)
    tw = R.trustworthiness(X, Y, 12)
    print('end to end sbm1024: dense fp64 KL %.4f (bar <= %.4f), trustworthiness %.4f (bar >= %.4f), KL on the sparse P %.4f'
          % (kl, kl_bar, tw, tw_bar, info['kl_divergence']))
    record_stat('t-SNE sbm1024 dense fp64 KL', '%.4f' % kl, '<= %.4f' % kl_bar)
    record_stat('t-SNE sbm1024 trustworthiness(12)', '%.4f' % tw, '>= %.4f' % tw_bar)
    assert info['n_iter'] == 1000
    assert kl <= kl_bar
    assert tw >= tw_bar


# ------------------------------------------------------------------ 7. refusals
def test_refusals():
    L = _hip.lib()
    X = np.ascontiguousarray(inputs('karate'))
    n, d = X.shape

    def create(n_, d_, ld_, X_, perplexity):
        h = C.c_void_p()
        rc = L.gemhip_tsne_create(n_, d_, ld_, _hip.ptr(X_, C.c_float), perplexity, C.byref(h))
        assert not h.value
        return rc, L.gemhip_last_error()

    rc, msg = create(n, d, d, X, 34.0)
    assert rc == _hip.E_INVALID and b'perplexity = 34 must be less than n = 34' in msg
    rc, msg = create(n, d, d, X, 50.0)
    assert rc == _hip.E_INVALID and b'must be less than n' in msg
    for bad in (4.9, 100.5, float('nan')):
        rc, msg = create(n, d, d, X, bad)
        assert rc == _hip.E_INVALID and b'outside [5, 100]' in msg
    rc, msg = create(n, 0, d, X, 10.0)
    assert rc == _hip.E_INVALID and b'd = 0' in msg
    rc, msg = create(n, d, d - 1, X, 10.0)
    assert rc == _hip.E_INVALID and b'ld = 3' in msg
    for bad in (np.nan, np.inf, -np.inf, 1e20):
        Xb = X.copy(); Xb[7, 2] = bad
        rc, msg = create(n, d, d, Xb, 10.0)
        assert rc == _hip.E_INVALID and b'X[7][2]' in msg
    with pytest.raises(_hip.GemHipError, match='outside'):
        tsne.tsne_2d(X, perplexity=3.0)
    # and a run without an embedding
    with tsne.TsneHandle(X, 10.0) as h:
        with pytest.raises(_hip.GemHipError, match='no embedding set'):
            h.run(1, 1.0, 0.5, 50.0)
        with pytest.raises(_hip.GemHipError, match='outside'):
            h.set_affinities(np.full((n, h.k), n, np.int32), np.zeros((n, h.k), np.float32))
