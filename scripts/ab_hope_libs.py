"""One HOPE / Laplacian Eigenmaps / LLE shape on the library GEM_HIP_LIB selects: sha256 of sigma, U, V (the solvers are deterministic: two builds of
the library must print the same ones), the integer statistics of the solve (SpMM launches and columns, basis size, cycles, host eigensolver calls)
and milliseconds per solve from stats[0] (median, min, max of REPS solves after a warm-up; host_eig_ms / spmm_ms: the last solve's shares).  Run it with two libraries in alternation, each in a
process of its own, to compare builds -- profiles/hope_host_refactor_ab.json was taken this way.  One JSON line.
    GEM_HIP_LIB=... python scripts/ab_hope_libs.py karate | sbm1024 | sbm2048_sym | sbm100k | sbm100k_directed | lap100k | lle100k
karate, sbm1024: block-Krylov; sbm2048_sym: SBM 2048/20480 with GEMHIP_HOPE_SYM=1; sbm100k: SBM 100k/1M, k = 64 (eigen-path); sbm100k_directed: the same
edges randomly oriented (block-Krylov with locking); lap100k / lle100k: gemhip_lap_eigmap / gemhip_lle on SBM 100k/1M (a solve includes its set-up)."""
import ctypes as C, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
shape = sys.argv[1]
if shape == 'sbm2048_sym':
    os.environ['GEMHIP_HOPE_SYM'] = '1'
import numpy as np
from gem_amd import _hip
from gem_amd.embedding.lap import symmetric_arrays
from gem_amd.graph import sbm_graph, orient_randomly, edge_arrays, to_csr

REPS, L = int(os.environ.get('REPS', 7)), _hip.lib()
if shape == 'karate':
    from gem_amd.utils import graph_util
    g, k = graph_util.loadGraphFromEdgeListTxt(os.path.join(ROOT, 'tests', 'golden', 'karate.edgelist'), directed=True).to_directed(), 2
elif shape == 'sbm1024':
    g, k = sbm_graph(1024, 10240, 8, seed=11), 16
elif shape == 'sbm2048_sym':
    g, k = sbm_graph(2048, 20480, 8, seed=11), 16
else:
    g, k = sbm_graph(100000, 1000000, 32, seed=20260925), 64
    if shape == 'sbm100k_directed':
        g = orient_randomly(g, 1)
one_sided = shape in ('lap100k', 'lle100k')
if one_sided:
    n, src, dst, w = symmetric_arrays(g)
    row_ptr, col, ww = to_csr(n, src, dst, w)
else:
    n, src, dst, w, _ = edge_arrays(g)
    row_ptr, col, ww = to_csr(n, src, dst, None)
rp, ci, wp = _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), _hip.ptr(ww, C.c_float)
U = np.zeros((n, k), np.float32); V = np.zeros((n, k), np.float32); s = np.zeros(k, np.float32)
stats = (C.c_double * 12)()
plan = C.c_void_p()
if not one_sided:
    _hip.check(L.gemhip_hope_plan_create(n, len(col), rp, ci, None, 0.01, C.byref(plan)))


def solve():
    if shape == 'lap100k':
        _hip.check(L.gemhip_lap_eigmap(n, len(col), rp, ci, wp, k, 16, 3, 30, 1e-6, 20260923, _hip.ptr(V, C.c_float), _hip.ptr(s, C.c_float), stats))
    elif shape == 'lle100k':
        _hip.check(L.gemhip_lle(n, len(col), rp, ci, wp, k, 16, 3, 40, 1e-6, 20260923, _hip.ptr(V, C.c_float), _hip.ptr(s, C.c_float), stats))
    else:
        _hip.check(L.gemhip_hope_plan_solve(plan, k, 16, 3, 20, 1e-5, 20260923, _hip.ptr(U, C.c_float), _hip.ptr(V, C.c_float), _hip.ptr(s, C.c_float), stats))
    return stats[0] * 1e3


ms = [solve() for _ in range(REPS + 1)][1:]                  # the first solve warms up
if not one_sided:
    _hip.check(L.gemhip_hope_plan_destroy(plan))
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
print(json.dumps(dict(shape=shape, lib=os.path.basename(_hip.LIB_PATH), sha256_sigma=sha(s), sha256_U=sha(U), sha256_V=sha(V), ms_per_solve=float(np.median(ms)),
                      ms_min=min(ms), ms_max=max(ms), spmm_launches=int(stats[1]), spmm_columns=int(stats[2]), katz_terms=int(stats[3]), basis_columns=int(stats[4]),
                      cycles=int(stats[5]), host_eig_calls=int(stats[9]), host_eig_ms=stats[8] * 1e3, spmm_ms=stats[11] * 1e3)), flush=True)
