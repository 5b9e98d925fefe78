"""The refusal cases of the evaluation units' create functions (gemhip_kmeans_create, _nc_create, _edgeclf_create, _tsne_create, _tsne_knn,
_nbr_create, _eval_create), shared by scripts/make_golden_eval_refusals.py (which records tests/golden/eval_units_refusals.txt) and
tests/test_eval_units_refusals.py (which compares the built library with that file).  Every refusal here is decided before the unit's first
HIP call, so the cases run without a device.

A case the host checks let through reaches the device: the call then returns GEMHIP_OK (a handle, destroyed at once) or, without a device,
GEMHIP_E_HIP.  Both are recorded as 'accepted' -- the text of a HIP failure names a source line and is not part of the record."""
import ctypes as C

import numpy as np

from gem_amd import _hip

N, D, LD = 8, 3, 4                  # the base matrix: 8 rows (t-SNE needs n > perplexity = 5), 3 columns and one of padding
PATH_RP, PATH_COL = [0, 1, 3, 4, 4, 4, 4, 4, 4], [1, 0, 2, 1]
ACCEPTED = 'accepted'


def base():
    return (np.arange(N * LD, dtype=np.float32).reshape(N, LD) - 11.0) / 8.0


def planted(value, at=(2, 1), then=None, then_at=None):
    X = base()
    X[at] = value
    if then_at is not None:
        X[then_at] = then
    return X


# unit -> (width limit or None, magnitude bound or None)
MATRIX_UNITS = {'kmeans_create': (256, None), 'nc_create': (255, None), 'edgeclf_create': (255, np.float32(1e18)), 'tsne_create': (None, np.float32(1e15)),
                'tsne_knn': (None, np.float32(1e15))}


def matrix_cases(unit):
    """[(what, n, d, ld, X or None, with an out pointer)] of one unit that takes (n, d, ld, X)."""
    max_d, max_abs = MATRIX_UNITS[unit]
    X = base()
    out = [('NULL out', N, D, LD, X, False),
           ('n = 0', 0, D, LD, X, True),
           ('n = 1', 1, D, LD, X, True),
           ('n = 2^31', 2 ** 31, D, LD, X, True),
           ('d = 0', N, 0, LD, X, True),
           ('ld < d', N, D, D - 1, X, True),
           ('NULL X', N, D, LD, None, True),
           ('NaN at X[2][1]', N, D, LD, planted(np.nan), True),
           ('+inf at X[2][1]', N, D, LD, planted(np.inf), True),
           ('-inf at X[2][1]', N, D, LD, planted(-np.inf), True),
           ('NaN in the last entry of the last row', N, D, LD, planted(np.nan, (N - 1, D - 1)), True),
           ('-inf in the last entry of the last row, d = ld', N, LD, LD, planted(-np.inf, (N - 1, LD - 1)), True),
           ('two offenders: +inf at X[1][2], NaN at X[2][0]', N, D, LD, planted(np.inf, (1, 2), np.nan, (2, 0)), True),
           ('NaN in the padding column X[2][3]', N, D, LD, planted(np.nan, (2, 3)), True),
           ('ld < d and NULL X', N, D, D - 1, None, True),
           ('n = 0 and d = 0', 0, 0, LD, X, True),
           ('d = 0 and NULL X', N, 0, LD, None, True)]
    if max_d is not None:
        out.append(('d one above the limit', N, max_d + 1, max_d + 1, X, True))          # refused before X is read
        out.append(('d one above the limit and NULL X', N, max_d + 1, max_d + 1, None, True))
        out.append(('d one above the limit and ld < d', N, max_d + 1, max_d, X, True))
    if max_abs is not None:
        above = np.nextafter(max_abs, np.float32(np.inf))
        out.append(('the magnitude bound itself at X[2][1]', N, D, LD, planted(max_abs), True))
        out.append(('minus the magnitude bound at X[2][1]', N, D, LD, planted(-max_abs), True))
        out.append(('the next float above the bound at X[2][1]', N, D, LD, planted(above), True))
        out.append(('minus the next float above the bound, last entry', N, D, LD, planted(-above, (N - 1, D - 1)), True))
        out.append(('above the bound at X[0][1], then NaN at X[0][2]', N, D, LD, planted(above, (0, 1), np.nan, (0, 2)), True))
    else:
        out.append(('the largest float at X[2][1]', N, D, LD, planted(np.finfo(np.float32).max), True))
    return out


def call_matrix(unit, case):
    """-> (rc, handle value or None, message)"""
    what, n, d, ld, X, with_out = case
    L = _hip.lib()
    h = C.c_void_p(1)
    out = C.byref(h) if with_out else None
    if unit == 'tsne_create':
        rc = L.gemhip_tsne_create(n, d, ld, _hip.ptr(X, C.c_float), 5.0, out)
    elif unit == 'tsne_knn':
        ids = np.zeros((N, 3), np.int32); dist = np.zeros((N, 3), np.float32)
        rc = L.gemhip_tsne_knn(n, d, ld, _hip.ptr(X, C.c_float), 3, _hip.ptr(ids, C.c_int32) if with_out else None, _hip.ptr(dist, C.c_float))
        h = C.c_void_p(0)
    else:
        rc = getattr(L, 'gemhip_' + unit)(n, d, ld, _hip.ptr(X, C.c_float), out)
    msg = L.gemhip_last_error().decode()
    if rc == 0 and h.value and with_out:
        getattr(L, 'gemhip_%s_destroy' % unit.split('_')[0])(h)
        h = C.c_void_p(0)
    return rc, h.value if with_out else None, msg


ARCS = (np.array([0, 1, 2, 2], np.int32), np.array([1, 2, 0, 3], np.int32))
# (what, n, m, src, dst, with an out pointer)
NBR_CASES = (('NULL out', 5, 4, ARCS[0], ARCS[1], False),
             ('n = 0', 0, 4, ARCS[0], ARCS[1], True),
             ('n = 2^31', 2 ** 31, 4, ARCS[0], ARCS[1], True),
             ('m = -1', 5, -1, ARCS[0], ARCS[1], True),
             ('NULL src', 5, 4, None, ARCS[1], True),
             ('NULL dst', 5, 4, ARCS[0], None, True),
             ('n = 0 and NULL src', 0, 4, None, ARCS[1], True),
             ('an arc to node n', 3, 4, ARCS[0], ARCS[1], True),
             ('a negative source', 5, 4, np.array([0, -1, 2, 2], np.int32), ARCS[1], True),
             ('INT32_MIN as a target', 5, 4, ARCS[0], np.array([1, 2, -2 ** 31, 9], np.int32), True),
             ('no arcs, NULL arrays', 5, 0, None, None, True),
             ('a valid graph', 5, 4, ARCS[0], ARCS[1], True))


def call_nbr(case):
    what, n, m, src, dst, with_out = case
    L = _hip.lib()
    h = C.c_void_p(1)
    rc = L.gemhip_nbr_create(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), C.byref(h) if with_out else None)
    msg = L.gemhip_last_error().decode()
    if rc == 0 and h.value and with_out:
        L.gemhip_nbr_destroy(h)
        h = C.c_void_p(0)
    return rc, h.value if with_out else None, msg


# (what, n, da, ld, A, kind, row_ptr, col, with an out pointer); tests/test_eval_host.py holds the CSR refusals
def eval_cases():
    X = base()
    return (('NULL out', N, D, LD, X, 0, PATH_RP, PATH_COL, False),
            ('n = 0', 0, D, LD, X, 0, PATH_RP, PATH_COL, True),
            ('n = 2^31', 2 ** 31, D, LD, X, 0, PATH_RP, PATH_COL, True),
            ('da = 0', N, 0, LD, X, 0, PATH_RP, PATH_COL, True),
            ('ld < da', N, D, D - 1, X, 0, PATH_RP, PATH_COL, True),
            ('da = 513', N, 513, 513, X, 0, PATH_RP, PATH_COL, True),
            ('NULL A', N, D, LD, None, 0, PATH_RP, PATH_COL, True),
            ('ld < da and NULL A', N, D, D - 1, None, 0, PATH_RP, PATH_COL, True),
            ('kind 2', N, D, LD, X, 2, PATH_RP, PATH_COL, True),
            ('NaN at A[2][1]', N, D, LD, planted(np.nan), 0, PATH_RP, PATH_COL, True),
            ('+inf at A[2][1]', N, D, LD, planted(np.inf), 0, PATH_RP, PATH_COL, True),
            ('-inf at A[2][1]', N, D, LD, planted(-np.inf), 0, PATH_RP, PATH_COL, True),
            ('NaN in the padding column A[2][3]', N, D, LD, planted(np.nan, (2, 3)), 0, PATH_RP, PATH_COL, True),
            ('a valid evaluator', N, D, LD, X, 0, PATH_RP, PATH_COL, True))


def call_eval(case):
    what, n, da, ld, A, kind, rp, col, with_out = case
    L = _hip.lib()
    rp = np.array(rp, np.int64); col = np.array(col, np.int32)
    h = C.c_void_p(1)
    rc = L.gemhip_eval_create(n, da, ld, _hip.ptr(A, C.c_float), None, kind, _hip.ptr(rp, C.c_int64), _hip.ptr(col, C.c_int32), C.byref(h) if with_out else None)
    msg = L.gemhip_last_error().decode()
    if rc == 0 and h.value and with_out:
        L.gemhip_eval_destroy(h)
        h = C.c_void_p(0)
    return rc, h.value if with_out else None, msg


def all_cases():
    """[(unit, what, thunk -> (rc, handle, message))] in the order of the golden file."""
    out = []
    for unit in MATRIX_UNITS:
        out += [(unit, case[0], lambda unit=unit, case=case: call_matrix(unit, case)) for case in matrix_cases(unit)]
    out += [('nbr_create', case[0], lambda case=case: call_nbr(case)) for case in NBR_CASES]
    out += [('eval_create', case[0], lambda case=case: call_eval(case)) for case in eval_cases()]
    return out


def record_line(unit, what, rc, handle, msg):
    """One line of the golden file.  A refusal leaves no handle behind; that is checked here, for the recorder and the test alike."""
    assert not handle, (unit, what, 'left a handle')
    if rc in (0, _hip.E_HIP):
        return '%s\t%s\t%s' % (unit, what, ACCEPTED)
    return '%s\t%s\t%d\t%s' % (unit, what, rc, msg)


def record():
    return [record_line(unit, what, *thunk()) for unit, what, thunk in all_cases()]


# ------------------------------------------------------------------ results: one SHA-256 per output array (scripts/digest_eval_units.py)
DIGEST_D, DIGEST_LD, DIGEST_SIZES, DIGEST_GRAPH_N = 20, 24, (1500, 70), 300
# 1500: above the 1024-thread one-workgroup sum and scan, so some threads take two elements and some one, and the scan carries once.
# 70: below one workgroup and no multiple of 64.  Columns 20 .. 23 are padding and hold NaN: no unit may read them.


def _sha(a):
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


def digest_matrix(n):
    X = np.random.RandomState(1000 + n).randn(n, DIGEST_LD).astype(np.float32)
    X[:, DIGEST_D:] = np.nan
    return X


def _kmeans(L, X, n, out):
    d, K, Kt = DIGEST_D, 7, 4
    h = C.c_void_p()
    _hip.check(L.gemhip_kmeans_create(n, d, DIGEST_LD, _hip.ptr(X, C.c_float), C.byref(h)))
    centres = np.ascontiguousarray(X[:K, :d]); labels = np.zeros(n, np.int32); info = np.zeros(6)
    _hip.check(L.gemhip_kmeans_fit(h, K, _hip.ptr(centres, C.c_float), 0.0, 5, _hip.ptr(labels, C.c_int32), _hip.ptr(info, C.c_double)))
    truth = np.random.RandomState(7).randint(0, Kt, size=n).astype(np.int32); table = np.zeros((K, Kt), np.int64)
    _hip.check(L.gemhip_kmeans_contingency(h, Kt, _hip.ptr(truth, C.c_int32), _hip.ptr(table, C.c_int64)))
    _hip.check(L.gemhip_kmeans_destroy(h))
    assert info[1] == 5 and table.sum() == n
    out.update({'kmeans.labels': _sha(labels), 'kmeans.centres': _sha(centres), 'kmeans.inertia': _sha(info[:1]), 'kmeans.contingency': _sha(table)})


def _tsne(L, X, n, out):
    d, k = DIGEST_D, 16                                              # k = floor(3 * perplexity) + 1
    ids = np.zeros((n, k), np.int32); dist = np.zeros((n, k), np.float32); p = np.zeros((n, k), np.float32)
    _hip.check(L.gemhip_tsne_knn(n, d, DIGEST_LD, _hip.ptr(X, C.c_float), k, _hip.ptr(ids, C.c_int32), _hip.ptr(dist, C.c_float)))
    _hip.check(L.gemhip_tsne_affinities(n, k, _hip.ptr(dist, C.c_float), 5.0, _hip.ptr(p, C.c_float)))
    h = C.c_void_p()
    _hip.check(L.gemhip_tsne_create(n, d, DIGEST_LD, _hip.ptr(X, C.c_float), 5.0, C.byref(h)))
    Y = (1e-4 * np.random.RandomState(3).randn(n, 2)).astype(np.float32)
    _hip.check(L.gemhip_tsne_set_embedding(h, _hip.ptr(Y, C.c_float)))
    grad = np.zeros((n, 2), np.float32); kl = C.c_double(); z = C.c_double()
    _hip.check(L.gemhip_tsne_gradient(h, 12.0, _hip.ptr(grad, C.c_float), C.byref(kl), C.byref(z)))
    kl_run = C.c_double(); gn = C.c_double()
    _hip.check(L.gemhip_tsne_run(h, 10, 12.0, 0.5, 200.0, C.byref(kl_run), C.byref(gn)))
    _hip.check(L.gemhip_tsne_get_embedding(h, _hip.ptr(Y, C.c_float)))
    _hip.check(L.gemhip_tsne_destroy(h))
    assert np.isfinite(kl.value) and z.value > 0 and np.all(np.isfinite(Y))
    out.update({'tsne.knn_id': _sha(ids), 'tsne.knn_dist': _sha(dist), 'tsne.affinities': _sha(p), 'tsne.gradient': _sha(grad),
                'tsne.kl': _sha(np.array([kl.value])), 'tsne.z': _sha(np.array([z.value])), 'tsne.embedding_after_10': _sha(Y),
                'tsne.kl_after_10': _sha(np.array([kl_run.value])), 'tsne.grad_norm_after_10': _sha(np.array([gn.value]))})


def _nc(L, X, n, out):
    d, K = DIGEST_D, 3
    rng = np.random.RandomState(11)
    member = rng.rand(n, K) < 0.4
    member[np.arange(n), rng.randint(0, K, size=n)] = True           # every row has a class; classes ascending within a row
    row_ptr = np.concatenate([[0], np.cumsum(member.sum(axis=1))]).astype(np.int64); cls = np.nonzero(member)[1].astype(np.int32)
    n_train = n * 2 // 3
    train = np.arange(n_train, dtype=np.int32); rest = np.arange(n_train, n, dtype=np.int32); m = len(rest)
    h = C.c_void_p()
    _hip.check(L.gemhip_nc_create(n, d, DIGEST_LD, _hip.ptr(X, C.c_float), C.byref(h)))
    _hip.check(L.gemhip_nc_set_labels(h, K, _hip.ptr(row_ptr, C.c_int64), _hip.ptr(cls, C.c_int32)))
    W = np.zeros((K, d + 1)); info = np.zeros((K, 6))
    _hip.check(L.gemhip_nc_fit(h, n_train, _hip.ptr(train, C.c_int32), 1.0, 1e-6, 50, _hip.ptr(W, C.c_double), _hip.ptr(info, C.c_double)))
    scores = np.zeros((m, K)); pred = np.zeros((m, K), np.uint8); counts = np.zeros(3 * K, np.int64); exact = np.zeros(1, np.int64)
    k_true = member[rest].sum(axis=1).astype(np.int32)
    _hip.check(L.gemhip_nc_scores(h, m, _hip.ptr(rest, C.c_int32), _hip.ptr(scores, C.c_double)))
    _hip.check(L.gemhip_nc_predict_topk(h, m, _hip.ptr(rest, C.c_int32), _hip.ptr(k_true, C.c_int32), _hip.ptr(pred, C.c_uint8), _hip.ptr(counts, C.c_int64),
                                        _hip.ptr(exact, C.c_int64)))
    _hip.check(L.gemhip_nc_destroy(h))
    assert np.all(np.isfinite(W)) and np.all(info[:, 4] == 1), info
    out.update({'nc.W': _sha(W), 'nc.scores': _sha(scores), 'nc.topk_pred': _sha(pred), 'nc.topk_counts': _sha(counts), 'nc.topk_exact': _sha(exact)})


def _edgeclf(L, X, n, out):
    d, m = DIGEST_D, 2000
    rng = np.random.RandomState(13)
    st = rng.randint(0, n, size=m).astype(np.int32); ed = rng.randint(0, n, size=m).astype(np.int32); label = (rng.rand(m) < 0.5).astype(np.uint8)
    h = C.c_void_p()
    _hip.check(L.gemhip_edgeclf_create(n, d, DIGEST_LD, _hip.ptr(X, C.c_float), C.byref(h)))
    for op, name in enumerate(('average', 'hadamard', 'l1', 'l2')):
        F = np.zeros((m, d), np.float32); w = np.zeros(d + 1); info = np.zeros(8); score = np.zeros(m)
        _hip.check(L.gemhip_edgeclf_features(h, op, m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(F, C.c_float)))
        _hip.check(L.gemhip_edgeclf_fit(h, op, m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(label, C.c_uint8), 1.0, 1e-6, 50, _hip.ptr(w, C.c_double),
                                        _hip.ptr(info, C.c_double)))
        _hip.check(L.gemhip_edgeclf_scores(h, op, m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(w, C.c_double), _hip.ptr(score, C.c_double)))
        assert np.all(np.isfinite(F)) and np.all(np.isfinite(w)) and np.all(np.isfinite(score))
        out.update({'edgeclf.%s.features' % name: _sha(F), 'edgeclf.%s.w' % name: _sha(w), 'edgeclf.%s.scores' % name: _sha(score)})
    dot = np.zeros(m)
    _hip.check(L.gemhip_edgeclf_scores(h, 0, m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), None, _hip.ptr(dot, C.c_double)))
    _hip.check(L.gemhip_edgeclf_destroy(h))
    out['edgeclf.dot'] = _sha(dot)


def digest_graph():
    """300 nodes, about 3000 distinct arcs without loops, as a CSR with ascending columns; a train mask of about half of them."""
    n = DIGEST_GRAPH_N
    rng = np.random.RandomState(17)
    A = rng.rand(n, n) < 3000.0 / (n * n)
    np.fill_diagonal(A, False)
    src, dst = np.nonzero(A)
    row_ptr = np.concatenate([[0], np.cumsum(A.sum(axis=1))]).astype(np.int64)
    T = A & (rng.rand(n, n) < 0.5)
    mask_rp = np.concatenate([[0], np.cumsum(T.sum(axis=1))]).astype(np.int64)
    return src.astype(np.int32), dst.astype(np.int32), row_ptr, mask_rp, np.nonzero(T)[1].astype(np.int32)


def _pairs(n, m, seed):
    rng = np.random.RandomState(seed)
    st = rng.randint(0, n, size=m).astype(np.int32)
    ed = ((st + 1 + rng.randint(0, n - 1, size=m)) % n).astype(np.int32)          # st != ed
    return st, ed


def _nbr(L, out):
    n, m = DIGEST_GRAPH_N, 2000
    src, dst, _, _, _ = digest_graph()
    st, ed = _pairs(n, m, 19)
    h = C.c_void_p()
    _hip.check(L.gemhip_nbr_create(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), C.byref(h)))
    cn = np.zeros(m, np.int32); jac, aa, ra, pa = (np.zeros(m) for _ in range(4))
    _hip.check(L.gemhip_nbr_scores(h, m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), 31, _hip.ptr(cn, C.c_int32), _hip.ptr(jac, C.c_double),
                                   _hip.ptr(aa, C.c_double), _hip.ptr(ra, C.c_double), _hip.ptr(pa, C.c_double)))
    _hip.check(L.gemhip_nbr_destroy(h))
    assert cn.max() > 0
    out.update({'nbr.cn': _sha(cn), 'nbr.jaccard': _sha(jac), 'nbr.aa': _sha(aa), 'nbr.ra': _sha(ra), 'nbr.pa': _sha(pa)})


def _eval(L, out):
    n, d, m, k = DIGEST_GRAPH_N, DIGEST_D, 2000, 10
    A = np.ascontiguousarray(digest_matrix(1500)[:n] * np.float32(0.25))
    _, col, row_ptr, mask_rp, mask_col = digest_graph()
    st, ed = _pairs(n, m, 23)
    st[:5] = ed[:5]                                                  # the zero diagonal
    nodes = np.arange(n, dtype=np.int32)
    for kind in (0, 1):
        h = C.c_void_p()
        _hip.check(L.gemhip_eval_create(n, d, DIGEST_LD, _hip.ptr(A, C.c_float), None, kind, _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), C.byref(h)))
        score = np.zeros(m); hit = np.zeros(m, np.uint8); ap = np.zeros(n); map_ = np.zeros(n); npos = np.zeros(n, np.int64)
        tid = np.zeros((n, k), np.int32); tscore = np.zeros((n, k)); thit = np.zeros((n, k), np.uint8)
        _hip.check(L.gemhip_eval_pairs(h, m, _hip.ptr(st, C.c_int32), _hip.ptr(ed, C.c_int32), _hip.ptr(score, C.c_double), _hip.ptr(hit, C.c_uint8)))
        _hip.check(L.gemhip_eval_ap(h, 0, n, _hip.ptr(nodes, C.c_int32), _hip.ptr(ap, C.c_double)))
        _hip.check(L.gemhip_eval_set_mask(h, _hip.ptr(mask_rp, C.c_int64), _hip.ptr(mask_col, C.c_int32)))
        _hip.check(L.gemhip_eval_ap_masked(h, 0, n, _hip.ptr(nodes, C.c_int32), _hip.ptr(map_, C.c_double), _hip.ptr(npos, C.c_int64)))
        _hip.check(L.gemhip_eval_topk(h, 0, 1, n, _hip.ptr(nodes, C.c_int32), k, _hip.ptr(tid, C.c_int32), _hip.ptr(tscore, C.c_double), _hip.ptr(thit, C.c_uint8)))
        _hip.check(L.gemhip_eval_destroy(h))
        assert hit.sum() > 0 and ap.max() > 0 and np.all(np.isfinite(score))
        tag = 'eval.kind%d.' % kind
        out.update({tag + 'pair_scores': _sha(score), tag + 'pair_hits': _sha(hit), tag + 'sampled_ap': _sha(ap), tag + 'masked_ap': _sha(map_),
                    tag + 'masked_npos': _sha(npos), tag + 'topk_id': _sha(tid), tag + 'topk_score': _sha(tscore), tag + 'topk_hit': _sha(thit)})


def digests():
    """{'<unit>.<output>[ n=<rows>]': sha256 of the array's bytes}.  Needs a device."""
    _hip.require_device()
    L = _hip.lib()
    out = {}
    for n in DIGEST_SIZES:
        X = digest_matrix(n)
        part = {}
        for unit in (_kmeans, _tsne, _nc, _edgeclf):
            unit(L, X, n, part)
        out.update(('%s n=%d' % (key, n), v) for key, v in part.items())
    _nbr(L, out)
    _eval(L, out)
    return out
