"""CPU tests of the schedules of the N-GPU entry points (gem_amd/csrc/multi_plan.hip) as plain C++ behind scripts/asan/multi_plan_driver.cpp: no HIP, no
device.  The same rules exist in gem_amd/multi_gpu.py (one process per GPU); the two implementations are held against each other here, integers
exactly and floats bit for bit.  The refusals the three entry points make before their first device call are also taken through the library and
compared with tests/golden/multi_refusals.txt, which records the library's texts from before the schedules moved out of multi.hip."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import golden_path
from gem_amd import _hip, build
from gem_amd.graph import edge_arrays
from gem_amd.multi_gpu import GFSharded, Node2VecPartitioned, TorchComm, shard_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, EDGE_OUT_OF_RANGE, NOT_ASCENDING = range(3)          # GfShardError::Kind
TOTALS, RANKS, EPISODES = (0, 1, 2, 5, 6, 1000, 1024), (1, 2, 3, 4, 7, 8, 64), (1, 3, 64)


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    d = tmp_path_factory.mktemp('multi_plan')
    exe = str(d / 'multi_plan_driver')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(ROOT, 'gem_amd', 'csrc', 'multi_plan.hip'),
                           os.path.join(ROOT, 'scripts', 'asan', 'multi_plan_driver.cpp'), '-o', exe])

    class Driver:
        def _lines(self, *args):
            out = subprocess.check_output([exe] + [str(a) for a in args])
            return [tuple(int(v) for v in line.split()) for line in out.decode().splitlines()]

        def shard(self, total, N):
            return self._lines('shard', total, N)

        def blocks(self, n, N):
            """(block, n_pad), [(r0, r1) of every rank]"""
            lines = self._lines('blocks', n, N)
            return lines[0], lines[1:]

        def n2v(self, total, N, episodes, walk_len, n, epochs):
            subprocess.check_call([exe, 'n2v'] + [str(a) for a in (total, N, episodes, walk_len, n, epochs, d / 'out')])
            raw = np.fromfile(d / 'out', np.int64)
            assert raw.size == 3 + 2 * N + 3 * episodes * N + episodes + epochs * episodes
            at = 3 + 2 * N
            return {'shard_rows': int(raw[0]), 'prow': int(raw[1]), 'alpha_total': int(raw[2]), 'shard': raw[3:at].reshape(N, 2),
                    'tab': raw[at:at + 3 * episodes * N].reshape(episodes, 3, N), 'seg_len': raw[at + 3 * episodes * N:at + 3 * episodes * N + episodes],
                    'token_offset': raw[at + 3 * episodes * N + episodes:].reshape(epochs, episodes)}

        def gfcheck(self, lists):
            """gf_check_shardable over [(n, src, dst)]: one (kind, edge, row, after) each."""
            with open(d / 'in', 'wb') as f:
                np.array([len(lists)], np.int64).tofile(f)
                for n, src, dst in lists:
                    np.array([n, len(src)], np.int64).tofile(f)
                    np.ascontiguousarray(src, np.int32).tofile(f); np.ascontiguousarray(dst, np.int32).tofile(f)
            subprocess.check_call([exe, 'gfcheck', str(d / 'in'), str(d / 'out')])
            return [tuple(int(v) for v in row) for row in np.fromfile(d / 'out', np.int64).reshape(len(lists), 4)]

        def parts(self, full, N):
            """partition_cut of every r (an [N, prow, d] array), and partition_paste of all of them into a NaN-filled table."""
            n, dd = full.shape
            with open(d / 'in', 'wb') as f:
                np.array([n, dd, N], np.int64).tofile(f)
                np.ascontiguousarray(full, np.float32).tofile(f)
            subprocess.check_call([exe, 'parts', str(d / 'in'), str(d / 'out')])
            raw = np.fromfile(d / 'out', np.float32)
            prow = (n + N - 1) // N
            assert raw.size == N * prow * dd + n * dd
            return raw[:N * prow * dd].reshape(N, prow, dd), raw[N * prow * dd:].reshape(n, dd)
    drv = Driver()
    drv.exe = exe
    return drv


def test_self_checks_pass(driver):
    run = subprocess.run([driver.exe, 'self'], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()[-3000:]


# ---------------------------------------------------------------------------------------------------------------- against gem_amd/multi_gpu.py
@pytest.mark.parametrize('N', RANKS)
def test_shard_range_is_multi_gpu_pys(driver, N):
    for total in TOTALS:
        assert driver.shard(total, N) == [shard_range(total, r, N) for r in range(N)], total


class _Backend(object):
    """What Node2VecPartitioned needs of a backend to plan and to walk through run(): it answers num_start_nodes() and records the bucket launches."""

    def __init__(self, total):
        self.total, self.launches = total, []

    def num_start_nodes(self):
        return self.total

    def walks(self, *a): pass
    def vocab(self): return None
    def gather_corpus(self, comm, shard_rows, world): return None
    def build_unigram_parts(self, *a): pass
    def upload_table(self, tab): return tab

    def init_part_tables(self, seed, rank, world):
        import torch
        return torch.zeros((1, 1)), None, None

    def train_part(self, corpus, seg_dev, e, nseg, seg_len, window, alpha0, alpha_total, token_offset, epoch, *rest):
        self.launches.append((epoch, e, seg_len, alpha_total, token_offset))

    def pairs(self, reset=True):
        return 0


class _Comm(object):
    def __init__(self, world): self.world = world
    def all_reduce_sum(self, t): pass
    def ring_shift(self, buf, tmp): return tmp, buf
    def all_gather_rows(self, full, own): full.zero_()


@pytest.mark.parametrize('episodes', EPISODES)
@pytest.mark.parametrize('N', RANKS)
def test_episode_table_and_alpha_are_node2vec_partitioneds(driver, N, episodes):
    """Shards, shard_rows, the [episodes][3][N] table and seg_len against episode_table(); alpha_total and the token offset in front of every episode
    against the arguments run() itself hands to every bucket launch (W = N ranks, rank 0's launches)."""
    walk_len, n, epochs = 8, 1001, 2
    for total in TOTALS + (2 * N * episodes,):                          # (6, 4, 3): empty slices; (2, 4): empty shards; the last: every slice 2 walks
        got = driver.n2v(total, N, episodes, walk_len, n, epochs)
        b = _Backend(total)
        py = Node2VecPartitioned(b, _Comm(N), 0, N, n, 1, walk_len, 3, epochs, 7, 11, episodes=episodes)
        tab, seg_len = py.episode_table()
        assert [tuple(s) for s in got['shard']] == [shard_range(total, r, N) for r in range(N)]
        assert got['shard_rows'] == py.shard_rows and got['prow'] == (n + N - 1) // N
        assert np.array_equal(got['tab'], tab) and np.array_equal(got['seg_len'], seg_len), total
        assert seg_len.min() >= 1
        py.run()
        assert len(b.launches) == epochs * episodes * N
        for k, (ep, e, sl, alpha_total, done) in enumerate(b.launches):
            assert (ep, e) == divmod(k // N, episodes)
            assert sl == got['seg_len'][e] and alpha_total == got['alpha_total'] and done == got['token_offset'][ep, e], (total, ep, e)
    if (N, episodes) == (4, 3):
        t = driver.n2v(6, 4, 3, walk_len, n, epochs)['tab']
        assert (t[:, 1] == 0).any() and t[:, 1].sum() == 6
    if N == 4:
        assert (np.diff(driver.n2v(2, 4, episodes, walk_len, n, epochs)['shard'], axis=1) == 0).sum() == 2


# ---------------------------------------------------------------------------------------------------------------- partitions, against numpy
@pytest.mark.parametrize('N', [1, 3, 4, 8])
def test_partition_cut_and_paste(driver, N):
    for n in (1, 5, 8, 1001):                                           # n = 1, 5 < N = 8: some partitions hold no row
        for d in (1, 16):
            full = np.random.RandomState(n + d).randn(n, d).astype(np.float32)
            parts, back = driver.parts(full, N)
            prow = (n + N - 1) // N
            for r in range(N):
                want = np.zeros((prow, d), np.float32)
                own = full[r::N]
                want[:len(own)] = own
                assert parts[r].tobytes() == want.tobytes(), (n, d, r)
            assert back.tobytes() == full.tobytes(), (n, d)


# ---------------------------------------------------------------------------------------------------------------- the GF rule
def _first_visits(src, dst):
    """Firing sources in the order the reference's sweep first visits them, and the edge of each first visit."""
    fire = np.flatnonzero(dst > src)
    rows, at = np.unique(src[fire], return_index=True)
    order = np.argsort(at)
    return rows[order], fire[at[order]]


def _gf_sharded_accepts(n, src, dst):
    try:
        GFSharded(None, TorchComm(1), 0, 2, n, src, dst)
        return True
    except ValueError:
        return False


def test_gf_rule_is_gf_shardeds_on_random_edge_lists(driver):
    rs = np.random.RandomState(5)
    lists = []
    for k in range(200):
        n, m = rs.randint(1, 13), rs.randint(0, 31)
        src, dst = rs.randint(0, n, m).astype(np.int32), rs.randint(0, n, m).astype(np.int32)
        perm = rs.permutation(m)                                        # shuffled edge order ...
        if k % 2:
            perm = perm[np.argsort(src[perm], kind='stable')]           # ... half of them grouped by ascending source again
        lists.append((n, src[perm], dst[perm]))
    got = driver.gfcheck(lists)
    accepted = 0
    for (n, src, dst), (kind, edge, row, after) in zip(lists, got):
        assert kind in (NONE, NOT_ASCENDING)
        assert (kind == NONE) == _gf_sharded_accepts(n, src, dst)
        accepted += kind == NONE
        if kind == NOT_ASCENDING:
            rows, at = _first_visits(src, dst)
            bad = np.flatnonzero(np.diff(rows) < 0)[0] + 1
            assert (edge, row, after) == (at[bad], rows[bad], rows[bad - 1])
        else:
            assert (edge, row, after) == (-1, -1, -1)
    assert accepted >= 40 and len(lists) - accepted >= 40, accepted


def test_gf_rule_on_karate_and_an_edge_out_of_range(driver, karate):
    n, src, dst, w, _ = edge_arrays(karate)
    order = np.lexsort((dst, src))
    bad_dst = dst[order].copy(); bad_dst[17] = n
    insertion, ascending, out_of_range = driver.gfcheck([(n, src, dst), (n, src[order], dst[order]), (n, src[order], bad_dst)])
    rows, at = _first_visits(src, dst)
    bad = np.flatnonzero(np.diff(rows) < 0)[0] + 1
    assert insertion == (NOT_ASCENDING, at[bad], rows[bad], rows[bad - 1]) and not _gf_sharded_accepts(n, src, dst)
    assert ascending == (NONE, -1, -1, -1) and _gf_sharded_accepts(n, src[order], dst[order])
    assert out_of_range == (EDGE_OUT_OF_RANGE, 17, -1, -1)


# ---------------------------------------------------------------------------------------------------------------- GF row blocks
@pytest.mark.parametrize('n,N', [(4, 4), (5, 4), (3, 4), (1001, 4), (1001, 1)])
def test_gf_row_blocks(driver, n, N):
    (block, n_pad), rows = driver.blocks(n, N)
    assert block == -(-n // N) and n_pad == block * N and n_pad % N == 0
    covered = np.zeros(n, np.int64)
    for r, (r0, r1) in enumerate(rows):
        assert r0 == min(r * block, n) and r1 == min((r + 1) * block, n)          # (an empty block is [n, n))
        covered[r0:r1] += 1
    assert np.all(covered == 1)
    for r in range(N):                                                   # ... and the blocks GFSharded gives its ranks
        py = GFSharded(None, TorchComm(1), r, N, n)
        assert (py.block, py.n_pad) == (block, n_pad) and (min(py.r0, n), max(min(py.r0, n), py.r1)) == rows[r]


# ---------------------------------------------------------------------------------------------------------------- refusals through the library
# (entry point, what, return code, arguments by name over the defaults below); tests/golden/multi_refusals.txt holds the library's text for each, in
# this order.  All of them precede the first device call, so this runs without a GPU.
PATH_SRC, PATH_DST = [0, 1, 2], [1, 2, 3]
REFUSALS = (('selftest', 'bytes not a multiple of 4', _hip.E_INVALID, dict(bytes=6)),
            ('selftest', 'bytes = 0', _hip.E_INVALID, dict(bytes=0)),
            ('selftest', 'bytes over 1 GiB', _hip.E_INVALID, dict(bytes=(1 << 30) + 4)),
            ('selftest', 'n_gpus = 0', _hip.E_INVALID, dict(n_gpus=0)),
            ('selftest', 'n_gpus = 65', _hip.E_INVALID, dict(n_gpus=65)),
            ('gf', 'no table', _hip.E_INVALID, dict(X=None)),
            ('gf', 'n = 0', _hip.E_INVALID, dict(n=0)),
            ('gf', 'max_iter < 0', _hip.E_INVALID, dict(max_iter=-1)),
            ('gf', 'd = 0', _hip.E_INVALID, dict(d=0)),
            ('gf', 'n_gpus = 0', _hip.E_INVALID, dict(n_gpus=0)),
            ('gf', 'n_gpus = -1', _hip.E_INVALID, dict(n_gpus=-1)),
            ('gf', 'n_gpus = 65', _hip.E_INVALID, dict(n_gpus=65)),
            ('gf', 'edge out of range', _hip.E_INVALID, dict(n_gpus=2, dst=[1, 2, 4])),
            ('gf', 'negative source', _hip.E_INVALID, dict(n_gpus=4, src=[-1, 1, 2])),
            ('gf', 'row 1 after row 2', _hip.E_UNSUPPORTED, dict(n_gpus=2, src=[0, 2, 1], dst=[1, 3, 2])),
            ('gf', 'row 0 after row 3', _hip.E_UNSUPPORTED, dict(n_gpus=64, n=5, src=[3, 4, 0], dst=[4, 0, 1])),
            ('gf', 'karate in insertion order', _hip.E_UNSUPPORTED, dict(n_gpus=2, karate=True)),
            ('n2v', 'no table', _hip.E_INVALID, dict(X=None)),
            ('n2v', 'episodes = 0', _hip.E_INVALID, dict(episodes=0)),
            ('n2v', 'epochs = 0', _hip.E_INVALID, dict(epochs=0)),
            ('n2v', 'epochs = 256', _hip.E_INVALID, dict(epochs=256)),
            ('n2v', 'n_gpus = 0', _hip.E_INVALID, dict(n_gpus=0)),
            ('n2v', 'n_gpus = 65', _hip.E_INVALID, dict(n_gpus=65)))


def library_refusal(case, karate):
    """The case through gemhip_rccl_selftest / gemhip_gf_train_multi / gemhip_n2v_train_multi: (return code, gemhip_last_error())."""
    entry, what, rc, over = case
    L = _hip.lib()
    a = dict(n=4, src=PATH_SRC, dst=PATH_DST, d=2, max_iter=1, n_gpus=1, bytes=4096, episodes=2, epochs=1, X=np.zeros((34, 2), np.float32))
    a.update(over)
    if a.get('karate'):
        a['n'], a['src'], a['dst'], _, _ = edge_arrays(karate)
    X = a['X']
    if entry == 'selftest':
        got = L.gemhip_rccl_selftest(a['n_gpus'], None, a['bytes'], None)
    elif entry == 'gf':
        src, dst = np.array(a['src'], np.int32), np.array(a['dst'], np.int32)
        got = L.gemhip_gf_train_multi(a['n'], len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), None, a['d'], 0.05, 0.01, a['max_iter'], a['n_gpus'], None,
                                      _hip.ptr(X, C.c_float), None)
    else:
        row_ptr, col = np.array([0, 1, 3, 5, 6], np.int64), np.array([1, 0, 2, 1, 3, 2], np.int32)
        got = L.gemhip_n2v_train_multi(4, len(col), _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), None, 2, 8, 1, 3, a['epochs'], 1.0, 1.0, 7, 11, a['n_gpus'], None,
                                       a['episodes'], _hip.ptr(X, C.c_float), None)
    return got, L.gemhip_last_error().decode()


def test_the_library_words_every_refusal_as_before(karate):
    want = open(golden_path('multi_refusals.txt')).read().splitlines()
    assert len(want) == len(REFUSALS)
    for case, text in zip(REFUSALS, want):
        rc, msg = library_refusal(case, karate)
        assert rc == case[2], case[:2]
        assert msg == text, case[:2]
