"""CPU tests of the SGNS launch rule (gemhip_sgns_plan_launch, gem_amd/csrc/sgns_plan.hip::plan_sgns_launch): host arithmetic, no device.

The reference has nothing to compare with -- the SNAP binary runs one Hogwild thread per core (gem/embedding/node2vec.py:34-53 passes no thread
count) -- so what is pinned here is the rule DESIGN.md 3.3 derives and the settings the GPU parity tests were measured at:
rho = W x 5 x w / n_eff <= 1.5 % (w = 0.4 pair steps with reload-on-update), n_eff over the cold rows once hot rows take atomic adds,
W <= 2 % of the rows that occur, n / (16 x 29) below 8192 nodes, at most 7 wavefronts per CU (LDS; 6 when a staging row for uncached contexts
is needed) x 256 CUs.
"""
import ctypes as C

import numpy as np
import pytest

from gem_amd import _hip


def plan(counts, d=128, window=10, walk_len=80, nwalks=None, flags=27):
    L = _hip.lib()
    counts = np.ascontiguousarray(counts, dtype=np.int32)
    k, w, hot = C.c_int32(), C.c_int32(), C.c_int32()
    ne, nec = C.c_double(), C.c_double()
    nwalks = int(counts.sum() // walk_len) if nwalks is None else nwalks
    _hip.check(L.gemhip_sgns_plan_launch(_hip.ptr(counts, C.c_int32), counts.size, d, window, walk_len, max(1, nwalks), flags,
                                         C.byref(k), C.byref(w), C.byref(hot), C.byref(ne), C.byref(nec)))
    return dict(kernel=k.value, waves=w.value, hot=hot.value, n_eff=ne.value, n_eff_cold=nec.value)


def zipf_counts(n, tokens, s=1.0, seed=0):
    r = np.random.RandomState(seed).permutation(n) + 1.0
    c = 1.0 / r ** s
    return np.maximum(1, np.round(c / c.sum() * tokens)).astype(np.int32)


def test_benchmark_shape_fills_the_device_without_hot_rows():
    """SBM 1M/10M (BASELINE configs[3]): equally frequent nodes -> n_eff = n, the rule allows 7500 wavefronts, the device holds 1792: with every
    context row cached the kernel needs 22 624 bytes of LDS per wavefront (tokens, targets, 21 rows as trained + 21 as loaded), seven per CU."""
    p = plan(np.full(1000000, 800), nwalks=10000000)
    assert p == dict(kernel=2, waves=1792, hot=0, n_eff=pytest.approx(1e6), n_eff_cold=pytest.approx(1e6))
    # a window shorter than the context radius needs the staging row for uncached contexts: six per CU
    assert plan(np.full(1000000, 800), nwalks=10000000, window=12)['waves'] == 1536
    # fewer walks than wavefronts: one wavefront per walk
    assert plan(np.full(1000000, 800), nwalks=100)['waves'] == 100


@pytest.mark.parametrize('n,waves', [(1024, 2), (4096, 8), (8192, 61), (16384, 122), (100000, 750), (400000, 1792)])
def test_uniform_graphs_follow_rho_and_the_small_graph_bound(n, waves):
    """rho <= 1.5 %: W = 0.015 n / (5 x 0.4); below 8192 nodes additionally n / (16 x 29) (tests/test_n2v_gpu.py measured SBM-1024 there)."""
    p = plan(np.full(n, 800))
    assert (p['kernel'], p['hot']) == (2, 0) and abs(p['waves'] - waves) <= 1        # (n_eff = z^2 / z2 rounds a hair below n)
    assert p['waves'] * 5 * 0.4 / p['n_eff'] <= 0.015 + 1e-12


def touch2(c):
    """sum_v (p_v + 5 q_v)^2: the collision rate of the rows a (centre, context) pair touches -- its context (token share p) and five negatives (q = unigram^0.75)"""
    c = np.asarray(c, dtype=np.float64)
    c = c[c > 0]
    u = c ** 0.75
    return float(((c / c.sum() + 5.0 * u / u.sum()) ** 2).sum())


def touch2_hub(c):
    """... minus what a table of equally frequent rows has (40 / active rows; an SBM: 38 / n): the part the hubs contribute, which the planner bounds"""
    return max(0.0, touch2(c) - 40.0 / max(1, int(np.count_nonzero(c))))


TOUCH_BOUND = 0.165          # (W - 1) x touch2_hub: sgns_plan.hip plan_sgns_launch, the conservative extrapolation of round 5 ...
TOUCH_FLOOR = 256            # ... which never takes a launch below 256 wavefronts (round 6: at 256 R-MAT scale 17 / 20 sit at -0.45 / -1.3 % of the oracle's MAP)


def bound_of(flags):
    return TOUCH_BOUND          # one bound for both unigram-table layouts (round 5 halved it for the node-id layout on two launches the heavy tail explains)


@pytest.mark.parametrize('flags', [27, 11])
@pytest.mark.parametrize('s', [0.6, 0.8, 1.0])
def test_power_law_counts_get_hot_rows_and_the_width_is_bounded_by_concurrent_touches(s, flags):
    """Zipf counts: hubs stay out of the LDS windows (hot rows: atomic updates), the cold rows carry the rho rule -- and, round 5, the width is bounded by
    the concurrent touches of one hub row, (W - 1) x touch2_hub <= 0.165: the bound that brought R-MAT scale 17 from -3.7 % to within 1 % and scale 20 from
    -6.4 % to within 2 % of the sequential MAP (tests/test_rmat_gpu.py, profiles/r05_rmat17_width_sweep.jsonl, r05_rmat20_launches_e128k.jsonl)."""
    n, tokens = 131072, 131072 * 800
    c = zipf_counts(n, tokens, s)
    p = plan(c, flags=flags)
    TOUCH_BOUND = bound_of(flags)
    assert p['kernel'] == 2 and p['hot'] >= 2
    assert p['n_eff'] < p['n_eff_cold'] and p['n_eff'] < 0.5 * n            # the hubs dominate the collision rate of the negative draws
    assert p['waves'] <= 0.015 * p['n_eff_cold'] / 2 + 1                    # rho over the cold rows
    assert p['waves'] <= 0.02 * np.count_nonzero(c) + 1                     # never more than 2 % of the rows that occur
    w_touch = max(TOUCH_FLOOR, 1 + int(TOUCH_BOUND / touch2_hub(c)))
    assert p['waves'] <= w_touch                                            # concurrent touches (never below the floor of 256 wavefronts)
    assert p['waves'] >= 0.85 * min(w_touch, 0.015 * p['n_eff_cold'] / 2, 768) - 1      # ... and no narrower than the rules ask (the search steps by 7/8; hot rows: at most 768)
    # hot = expected to sit in another wavefront's window: count >= tokens / ((W - 1)(2R + 1))
    assert p['hot'] == max(2, int(np.ceil(c.sum() / ((p['waves'] - 1) * 21.0))))
    assert (c >= p['hot']).sum() < 0.02 * n


def test_the_measured_rmat_corpora():
    """Token-count summaries of the graphs the rule was measured on (scripts/check_rmat17_launches.py --save-counts): R-MAT scale 17 and 20 -> the floor of
    256 wavefronts (the bound alone: 50 / 207 -- round 5's widths; measured in round 6 with the heavy tail gone: -0.45 % / -1.3 % of the oracle's MAP at 256,
    -1.6 / -3.0 % at 768), scale 22 (BASELINE configs[4]) -> 548 by the bound (round 4: 1536); launches with hot rows are capped at 768 wavefronts anyway
    (their atomic updates saturate: scale 22 33.0 s at 768 against 36.7 s at 1536).  SBM 1M/10M (no hubs) keeps 1792.  Both unigram-table layouts plan alike."""
    import json, os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rmat_token_count_histograms.json')
    H = json.load(open(path))
    for name, want, want_node_id in (('rmat17', 256, 256), ('rmat20', 256, 256), ('rmat22', 548, 548)):
        h = H[name]
        c = np.repeat(np.asarray(h['count'], dtype=np.int64), np.asarray(h['nodes'], dtype=np.int64)).astype(np.int32)
        c = np.concatenate([c, np.zeros(h['n'] - len(c), np.int32)])
        for flags, w in ((27, want), (11, want_node_id)):                   # the plugin default (the binary's table layout) / the node-id layout: the same plan
            p = plan(c, nwalks=h['nwalks'], flags=flags)
            assert p['waves'] == w and p['hot'] > 0, (name, flags, p)
            assert p['waves'] == TOUCH_FLOOR or (p['waves'] - 1) * touch2_hub(c) <= bound_of(flags) + 1e-9
            assert p['waves'] * 5 * 0.4 / p['n_eff_cold'] <= 0.015
    assert touch2_hub(np.full(1000000, 800)) == 0.0                         # equally frequent rows: the bound does not apply


def test_rows_that_never_occur_do_not_count():
    """Half of the table never appears in a walk (isolated nodes): the 2 % bound is over the active rows."""
    c = np.zeros(200000, dtype=np.int32)
    c[::2] = 800
    p = plan(c)
    assert p['n_eff'] == pytest.approx(100000.0) and abs(p['waves'] - 750) <= 1


def test_deterministic_and_fallback_launches():
    c = np.full(20000, 800)
    assert plan(c, flags=11 | 4) == dict(kernel=1, waves=1, hot=0, n_eff=pytest.approx(20000.0), n_eff_cold=pytest.approx(20000.0))
    # rows too wide for two copies of a 21-row window in 64 KB of LDS: the kernel without the window, n / 128 wavefronts
    p = plan(c, d=384)
    assert (p['kernel'], p['waves']) == (0, 20000 // 128)
    assert plan(c, d=256)['kernel'] == 2 and plan(c, d=182)['kernel'] == 2 and plan(c, d=255)['kernel'] == 2
    # the window-cache opt-out flag of gem_hip.h
    assert plan(c, flags=11 | _hip.N2V_NO_WINDOW_CACHE)["kernel"] == 0


def test_bad_arguments():
    L = _hip.lib()
    assert L.gemhip_sgns_plan_launch(None, 10, 128, 10, 80, 1, 11, None, None, None, None, None) != 0
    c = np.ones(4, dtype=np.int32)
    assert L.gemhip_sgns_plan_launch(_hip.ptr(c, C.c_int32), 4, 0, 10, 80, 1, 11, None, None, None, None, None) != 0
    assert L.gemhip_sgns_plan_launch(_hip.ptr(c, C.c_int32), 4, 16, 10, 80, 1, 11, None, None, None, None, None) == 0


def test_stand_alone_driver_reproduces_the_recorded_grid_and_the_oracle_tables(tmp_path, sbm1024):
    """gem_amd/csrc/sgns_plan.hip as plain C++ behind scripts/asan/plan_driver.cpp (no HIP, no library): the launch-rule grid -- every knob, bucket_knobs
    for 1 / 2 / 4 / 8 partitions -- byte for byte as recorded before the rule moved out of n2v.hip (tests/golden/sgns_plan_grid.txt, CHANGELOG.md), the
    invariants of the unified table builder on small inputs (the driver's exit status), and that builder's tables on the SBM-1024 corpus of the CPU
    oracle against the oracle's four builders: the same integers, the same fp32 bits."""
    import os
    import subprocess
    import oracle
    from gem_amd import build
    from gem_amd.graph import edge_arrays
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    exe = str(tmp_path / 'plan_driver')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(root, 'gem_amd', 'csrc', 'sgns_plan.hip'),
                           os.path.join(root, 'scripts', 'asan', 'plan_driver.cpp'), '-o', exe])
    golden = os.path.join(root, 'tests', 'golden')
    run = subprocess.run([exe, 'grid', os.path.join(golden, 'rmat_token_count_histograms.json')], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-2000:]
    assert run.stdout == open(os.path.join(golden, 'sgns_plan_grid.txt'), 'rb').read()

    def tables(counts, order, parts, flags):
        n = len(counts)
        with open(tmp_path / 'in', 'wb') as f:
            np.array([n, parts, flags, order is not None], np.int32).tofile(f)
            np.ascontiguousarray(counts, np.int32).tofile(f)
            if order is not None:
                np.ascontiguousarray(order, np.int32).tofile(f)
        subprocess.check_call([exe, 'tables', str(tmp_path / 'in'), str(tmp_path / 'out')])
        with open(tmp_path / 'out', 'rb') as f:
            rc = int(np.fromfile(f, np.int32, 1)[0]); n_vocab = int(np.fromfile(f, np.int64, 1)[0])
            U = np.fromfile(f, np.float32, n); K = np.fromfile(f, np.int32, n); slot = np.fromfile(f, np.int32, n)
            off = np.fromfile(f, np.int64, parts + 1); nslots = np.fromfile(f, np.int64, parts)
        assert rc == -1
        return n_vocab, U, K, slot, off, nslots

    n, src, dst, w, _ = edge_arrays(sbm1024)
    row_ptr, col, _ = oracle.sorted_csr(n, src, dst, w)
    walks = oracle.n2v_walks(row_ptr, col, None, None, 1.0, 1.0, 2, 20, 5, 11)
    walks[1::7, 10:] = -1                                         # padded tails, as the shorter shards of a gathered corpus have them
    counts = oracle.n2v_vocab(n, walks)
    gone = int(counts.argmax())                                   # ... and a node the corpus does not name (its tokens: padding)
    walks[walks == gone] = -1
    counts = oracle.n2v_vocab(n, walks)
    assert np.flatnonzero(counts == 0).tolist() == [gone]
    flat = walks.ravel()
    first = np.full(n, flat.size, np.int64)
    np.minimum.at(first, flat[flat >= 0], np.flatnonzero(flat >= 0))
    order = np.argsort(first, kind='stable').astype(np.int32)     # first-appearance order, the node that never occurs last
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    for parts in (1, 2, 4):
        # node-id layout: Vose over every row of a partition, in id order
        n_vocab, U, K, slot, off, nslots = tables(counts, None, parts, 11)
        UT, KT, ooff = oracle.unigram_build_parts(counts, parts)
        assert list(off) == list(ooff) and n_vocab == n and list(nslots) == list(np.diff(ooff)) and np.all(slot == -1)
        assert np.array_equal(bits(U), bits(UT)) and np.array_equal(K, KT)
        if parts == 1:
            UT1, KT1 = oracle.unigram_build(counts)
            assert np.array_equal(bits(U), bits(UT1)) and np.array_equal(K, KT1)
        # the binary's layout: the partition's nodes that occur, in first-appearance order; with and without RndUnigramInt's quirk in the slot table
        for flags in (27, 25):
            n_vocab, U, K, slot, off, nslots = tables(counts, order, parts, flags)
            want = oracle.unigram_build_parts_vocab_order(counts, walks, parts, flags)
            assert n_vocab == n - 1 == int(nslots.sum())
            for p, (st, UTp, KTp) in enumerate(want):
                a, b = int(off[p]), int(off[p + 1])
                assert nslots[p] == len(st) and np.array_equal(slot[a:a + len(st)], st) and np.all(slot[a + len(st):b] == -1)
                assert np.array_equal(bits(U[a:b]), bits(UTp)) and np.array_equal(K[a:b], KTp)
            if parts == 1:
                st1, UTn, KTn = oracle.unigram_build_vocab_order(counts, walks, flags)[:3]
                assert np.array_equal(slot[:len(st1)], st1) and np.array_equal(bits(U), bits(UTn)) and np.array_equal(K, KTn)
