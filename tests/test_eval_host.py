"""CPU tests of the evaluator's device-free host half (gem_amd/csrc/eval_host.hip: check_eval_csr, normalise_mask, ap_chunks, ap_from_counts) as
plain C++ behind scripts/asan/eval_host_driver.cpp: no HIP, no device.  Everything but AP itself is integer and must be exact; AP is held to
instrument_refs.AP_GRID_BAR on the half-integer grid family, where every score is exact and ties are decided by id.  The refusals of
gemhip_eval_create are also taken through the library: it makes them before its first HIP call, and words them as
tests/golden/eval_create_refusals.txt records from the library before the check moved out of eval.hip.

EVAL_HOST_DRIVER=<program> runs the same tests through a driver built elsewhere (scripts/build_asan_eval.sh: with AddressSanitizer and UBSan)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import instrument_refs as ir
import linkpred_refs as lr
from conftest import golden_path
from gem_amd import _hip, build
from gem_amd.evaluation import link_prediction as lp
from gem_amd.evaluation import reconstruction as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, ROW_PTR_FIRST, ROW_PTR_DECREASES, COL_NULL, COLUMN_OUT_OF_RANGE = range(5)          # EvalCsrError::Kind
EV_MAXNB = 512
N = ir.AP_N


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp('eval_host')
    exe = os.environ.get('EVAL_HOST_DRIVER')
    if not exe:
        hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
        cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
                   if os.path.exists(c))
        exe = str(d / 'eval_host_driver')
        subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(ROOT, 'gem_amd', 'csrc', 'eval_host.hip'),
                               os.path.join(ROOT, 'scripts', 'asan', 'eval_host_driver.cpp'), '-o', exe])

    def run(mode, *parts):
        with open(d / 'in', 'wb') as f:
            for part in parts:
                part.tofile(f)
        subprocess.check_call([exe, mode, str(d / 'in'), str(d / 'out')])
        return open(d / 'out', 'rb').read()

    def i64(*v):
        return np.array(v, np.int64)

    def csr(row_ptr, col):
        return np.ascontiguousarray(row_ptr, np.int64), np.zeros(0, np.int32) if col is None else np.ascontiguousarray(col, np.int32)

    class Driver:
        def check(self, n, row_ptr, col):
            """check_eval_csr: (kind, index, column, sorted); sorted is -1 on a refusal."""
            rp, c = csr(row_ptr, col)
            return tuple(int(v) for v in np.frombuffer(run('check', i64(n, -1 if col is None else len(c)), rp, c), np.int64))

        def mask(self, n, row_ptr, col):
            rp, c = csr(row_ptr, col)
            raw = run('mask', i64(n, len(c)), rp, c)
            out_rp = np.frombuffer(raw, np.int64, n + 1)
            return out_rp, np.frombuffer(raw, np.int32, int(out_rp[n]), 8 * (n + 1))

        def chunks(self, n, row_ptr, col, mask, undirected, nodes):
            """ap_chunks: a dict of ApChunks' five arrays.  mask: None or normalise_mask's (row_ptr, col)."""
            rp, c = csr(row_ptr, col)
            nodes = np.ascontiguousarray(nodes, np.int32)
            raw = run('chunks', i64(n, len(c), -1 if mask is None else len(mask[1]), int(undirected), len(nodes)), rp, c, *(() if mask is None else csr(*mask)), nodes)
            total, nchunk = (int(v) for v in np.frombuffer(raw, np.int64, 2))
            at, out = 16, {}
            for name, dtype, count in (('node_off', np.int64, len(nodes) + 1), ('chunk_off', np.int64, nchunk), ('nb', np.int32, total),
                                       ('chunk_node', np.int32, nchunk), ('chunk_cnt', np.int32, nchunk)):
                out[name] = np.frombuffer(raw, dtype, count, at); at += count * np.dtype(dtype).itemsize
            assert at == len(raw)
            return out

        def ap(self, node_off, nb, score, count, want_npos=True):
            ns = len(node_off) - 1
            raw = run('ap', i64(ns, len(nb), int(want_npos)), np.ascontiguousarray(node_off, np.int64), np.ascontiguousarray(score, np.float64),
                      np.ascontiguousarray(nb, np.int32), np.ascontiguousarray(count, np.int32))
            return np.frombuffer(raw, np.float64, ns), np.frombuffer(raw, np.int64, ns, 8 * ns)
    return Driver()


@functools.lru_cache(maxsize=None)
def graph():
    row_ptr, col, truth = ir.ap_graph()
    mrp, mcol, train = lr.lp_mask(truth)
    return row_ptr, col, truth, mrp, mcol, train


def positives(i, row_ptr, col, undirected, train_row):
    """sorted(set(row) - {i} - lower ids if undirected - mask row)"""
    row = np.unique(col[row_ptr[i]:row_ptr[i + 1]])
    row = row[(row != i) & ~(undirected & (row < i))]
    return row if train_row is None else row[~train_row[row]]


# ------------------------------------------------------------------ ap_chunks
SAMPLE = np.concatenate([np.arange(N), [ir.AP_HUB, ir.AP_HUB, ir.AP_513, ir.AP_EMPTY, 0]]).astype(np.int32)       # all 700 nodes, then repeats


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('undirected', [False, True])
def test_ap_chunks_are_the_numpy_restatement(driver, undirected, masked):
    row_ptr, col, truth, mrp, mcol, train = graph()
    got = driver.chunks(N, row_ptr, col, driver.mask(N, mrp, mcol) if masked else None, undirected, SAMPLE)
    want = [positives(i, row_ptr, col, undirected, train[i] if masked else None) for i in SAMPLE]
    node_off = np.concatenate([[0], np.cumsum([len(w) for w in want])])
    assert np.array_equal(got['node_off'], node_off) and np.all(np.diff(got['node_off']) >= 0)
    assert np.array_equal(got['nb'], np.concatenate(want))
    cn, co, cc = [], [], []
    for k, (i, w) in enumerate(zip(SAMPLE, want)):
        for o in range(0, len(w), EV_MAXNB):                          # the node's own slice, cut at 512; none for a node without positives
            cn.append(i); co.append(node_off[k] + o); cc.append(min(EV_MAXNB, len(w) - o))
    assert np.array_equal(got['chunk_node'], cn) and np.array_equal(got['chunk_off'], co) and np.array_equal(got['chunk_cnt'], cc)

    def cnt_of(k):                                                    # chunk sizes of the k-th sampled entry
        inside = (got['chunk_off'] >= node_off[k]) & (got['chunk_off'] < node_off[k + 1])
        assert np.all(got['chunk_node'][inside] == SAMPLE[k])
        return list(got['chunk_cnt'][inside])
    assert cnt_of(ir.AP_EMPTY) == [] and (not undirected or cnt_of(ir.AP_LOWER) == [])
    assert cnt_of(ir.AP_HUB) == [512, 88]                             # the hub's mask row is empty
    assert cnt_of(N) == cnt_of(N + 1) == [512, 88] and node_off[N + 1] - node_off[N] == 600 and node_off[N + 2] - node_off[N + 1] == 600      # repeats: slices of their own
    if not masked:
        assert cnt_of(ir.AP_512) == [512] and cnt_of(ir.AP_513) == [512, 1] and cnt_of(N + 2) == [512, 1]
        assert list(want[ir.AP_TWICE]) == ([21, 333, 400] if undirected else [17, 21, 333, 400])      # unsorted row, column 400 twice
    else:
        assert cnt_of(ir.AP_512) == [112] and cnt_of(lr.LP_ALL_MASKED) == []      # 400 of node 5's neighbours are train arcs


# ------------------------------------------------------------------ ap_from_counts
@functools.lru_cache(maxsize=None)
def grid_scores(da, kind):
    A, B = ir.ap_operands(da, 0, kind, False, 'grid', seed=ir.ap_seed(da, kind))
    score, _ = ir.ap_dense_scores(A, B, da, kind)
    score.setflags(write=False)
    return score


def streamed_counts(score_row, i, nb, undirected, train_row):
    """The kernel's count for every neighbour t in nb: candidates j (j != i, j > i when undirected, not a mask arc, s_j > 0) with
    s_j > s_t or (s_j == s_t and j < t)."""
    ok = score_row > 0
    ok[i] = False
    if undirected:
        ok[:i] = False
    if train_row is not None:
        ok &= ~train_row
    j = np.flatnonzero(ok)
    sj, st = score_row[j][None, :], score_row[nb][:, None]
    return ((sj > st) | ((sj == st) & (j[None, :] < nb[:, None]))).sum(axis=1)


assert (1, 0, 0, False) in ir.AP_CASES and (63, 0, 1, False) in ir.AP_CASES


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('da,kind', [(1, 0), (63, 1)])
def test_ap_from_counts_end_to_end(driver, da, kind, masked):
    row_ptr, col, truth, mrp, mcol, train = graph()
    score = grid_scores(da, kind)
    nodes = np.arange(N, dtype=np.int32)
    for undirected in (True, False):
        c = driver.chunks(N, row_ptr, col, driver.mask(N, mrp, mcol) if masked else None, undirected, nodes)
        s = np.concatenate([score[i, c['nb'][c['node_off'][i]:c['node_off'][i + 1]]] for i in nodes])
        count = np.concatenate([streamed_counts(score[i], i, c['nb'][c['node_off'][i]:c['node_off'][i + 1]].astype(np.int64), undirected, train[i] if masked else None)
                                for i in nodes])
        ap, npos = driver.ap(c['node_off'], c['nb'], s, count)
        ref = lp.link_prediction_rows(score, train, truth, undirected=undirected) if masked else gr.average_precision_rows(score, truth, undirected=undirected)
        err = np.abs(ap - ref)
        print('da=%d kind=%d masked=%d undirected=%d: max |AP - ref| = %.3g at node %d, MAP %.6f' % (da, kind, masked, undirected, err.max(), int(err.argmax()), ap.mean()))
        assert np.all(err <= ir.AP_GRID_BAR) and ap.max() > 0
        assert np.array_equal(npos, lr.npos_reference(score, train if masked else np.zeros_like(train), truth, undirected))
        again, none = driver.ap(c['node_off'], c['nb'], s, count, want_npos=False)                 # npos_out may be null
        assert again.tobytes() == ap.tobytes() and np.all(none == -7)


# ------------------------------------------------------------------ normalise_mask
def test_normalise_mask_sorts_and_drops_repeats(driver):
    rows = [[5, 1, 5, 3, 1], [], [0], [6, 6, 6], [2, 1, 0], [], [4, 0, 4]]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    out_rp, out_col = driver.mask(len(rows), rp, np.concatenate(rows))
    want = [np.unique(r) for r in rows]
    assert np.array_equal(out_rp, np.concatenate([[0], np.cumsum([len(w) for w in want])])) and np.array_equal(out_col, np.concatenate(want))
    out_rp, out_col = driver.mask(3, [0, 0, 0, 0], None)
    assert not out_rp.any() and out_col.size == 0
    _, _, truth, mrp, mcol, train = graph()                                                   # the train mask of the GPU tests
    out_rp, out_col = driver.mask(N, mrp, mcol)
    assert all(np.array_equal(out_col[out_rp[i]:out_rp[i + 1]], np.flatnonzero(train[i])) for i in range(N))


# ------------------------------------------------------------------ check_eval_csr
PATH_RP, PATH_COL = [0, 1, 3, 4], [1, 0, 2, 1]


def test_check_eval_csr(driver):
    assert driver.check(3, PATH_RP, PATH_COL) == (NONE, -1, 0, 1)
    assert driver.check(3, [0, 0, 0, 0], None) == (NONE, -1, 0, 1)                            # no edge needs no columns
    assert driver.check(3, [1, 1, 3, 4], PATH_COL)[:2] == (ROW_PTR_FIRST, 0)
    assert driver.check(3, [0, 3, 1, 4], PATH_COL)[:2] == (ROW_PTR_DECREASES, 1)
    assert driver.check(3, PATH_RP, None)[0] == COL_NULL
    assert driver.check(3, PATH_RP, [1, 0, 3, -1])[:3] == (COLUMN_OUT_OF_RANGE, 2, 3)
    assert driver.check(3, PATH_RP, [1, 0, 2, -1])[:3] == (COLUMN_OUT_OF_RANGE, 3, -1)
    assert driver.check(3, [0, 3, 1, 4], [1, 0, 3, 1])[:2] == (ROW_PTR_DECREASES, 1)          # row_ptr is looked at before the columns
    assert driver.check(3, [1, 0, 3, 4], None)[0] == ROW_PTR_FIRST
    assert driver.check(3, PATH_RP, [1, 2, 0, 1])[3] == 0                                     # a descending pair inside row 1
    assert driver.check(3, PATH_RP, [1, 2, 2, 0])[3] == 1                                     # equal neighbours; a descent across a row boundary is none
    row_ptr, col, _, _, _, _ = graph()
    assert driver.check(N, row_ptr, col) == (NONE, -1, 0, 0)                                  # row 20 of ap_graph is unsorted


# ------------------------------------------------------------------ the library's wording
X3 = np.full((3, 4), 0.5, np.float32)
# (what, n, da, ld, A, B, kind, row_ptr, col, with an out pointer); tests/golden/eval_create_refusals.txt holds the library's text for each, in this order
REFUSALS = (('out is null', 3, 3, 4, X3, None, 0, PATH_RP, PATH_COL, False),
            ('n = 0', 0, 3, 4, X3, None, 0, PATH_RP, PATH_COL, True),
            ('da above 512', 3, 513, 513, X3, None, 0, PATH_RP, PATH_COL, True),
            ('ld below da', 3, 3, 2, X3, None, 0, PATH_RP, PATH_COL, True),
            ('no embedding', 3, 3, 4, None, None, 0, PATH_RP, PATH_COL, True),
            ('no row_ptr', 3, 3, 4, X3, None, 0, None, PATH_COL, True),
            ('kind 2', 3, 3, 4, X3, None, 2, PATH_RP, PATH_COL, True),
            ('kind 1 with a second operand', 3, 3, 4, X3, X3.copy(), 1, PATH_RP, PATH_COL, True),
            ('row_ptr[0] != 0', 3, 3, 4, X3, None, 0, [1, 1, 3, 4], PATH_COL, True),
            ('row_ptr decreases', 3, 3, 4, X3, None, 0, [0, 3, 1, 4], PATH_COL, True),
            ('row_ptr decreases and a column is out of range', 3, 3, 4, X3, None, 0, [0, 3, 1, 4], [1, 0, 3, 1], True),
            ('col is null', 3, 3, 4, X3, None, 0, PATH_RP, None, True),
            ('column 3 of 3, then -1', 3, 3, 4, X3, None, 0, PATH_RP, [1, 0, 3, -1], True),
            ('column -1', 3, 3, 4, X3, None, 0, PATH_RP, [1, 0, 2, -1], True))


def library_refusal(case):
    """gemhip_eval_create on the case: (return code, handle, gemhip_last_error())."""
    what, n, da, ld, A, B, kind, rp, col, with_out = case
    L = _hip.lib()
    rp = None if rp is None else np.array(rp, np.int64)
    col = None if col is None else np.array(col, np.int32)
    h = C.c_void_p(1)
    rc = L.gemhip_eval_create(n, da, ld, _hip.ptr(A, C.c_float), _hip.ptr(B, C.c_float), kind, _hip.ptr(rp, C.c_int64), _hip.ptr(col, C.c_int32),
                              C.byref(h) if with_out else None)
    return rc, h.value if with_out else None, L.gemhip_last_error().decode()


def test_the_library_words_every_refusal_as_before():
    """Every refusal of gemhip_eval_create precedes its first HIP call, so this runs without a GPU."""
    want = open(golden_path('eval_create_refusals.txt')).read().splitlines()
    assert len(want) == len(REFUSALS)
    for case, text in zip(REFUSALS, want):
        rc, h, msg = library_refusal(case)
        assert rc == _hip.E_INVALID and not h, case[0]
        assert msg == text, case[0]
