"""One GF shape on the library GEM_HIP_LIB selects: a digest of the table after 5 sweeps from a fixed start (GF is deterministic: two builds of the
library must print the same one) and microseconds per sweep (median of REPS timed blocks).  Run it with two libraries in alternation, each in a process
of its own, to compare builds -- profiles/gf_refactor_ab.json was taken this way.  One JSON line.
    GEM_HIP_LIB=... python scripts/ab_gf_libs.py sbm1m | sbm10k | sbm10k_fused8 | sbm10k_halves | rmat<scale>
sbm1m: SBM 1M/10M (gf_sweep_rows_kernel); sbm10k: SBM 10k/100k (gf_sweep_kernel), _fused8: 8 sweeps per cooperative launch (gf_sweeps_coop_kernel),
_halves: as two sorted halves (the unit kernels, small levels fused); rmat<scale>: R-MAT, 16 edges per node (gf_hub_kernel beside the sweep)."""
import ctypes as C, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np
from gem_amd import _hip
from gem_amd.graph import sbm_graph, rmat_graph, edge_arrays

shape = sys.argv[1]
D, REPS, L = 128, int(os.environ.get('REPS', 7)), _hip.lib()
if shape.startswith('rmat'):
    g = rmat_graph(int(shape[4:]), 16 << int(shape[4:]), seed=20260923 + 5)
    sweeps = 20
elif shape == 'sbm1m':
    g = sbm_graph(1000000, 10000000, 100, seed=20260923 + 4)
    sweeps = 50
else:
    g = sbm_graph(10000, 100000, 10, seed=20260923 + 4)
    sweeps = 1000
n, src, dst, w, _ = edge_arrays(g)
if shape == 'sbm10k_halves':
    pick = np.random.RandomState(3).rand(len(src)) < 0.5
    perm = np.concatenate([np.flatnonzero(pick), np.flatnonzero(~pick)])
    src, dst = np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm])
m = len(src)
plan = C.c_void_p()
_hip.check(L.gemhip_gf_plan_create_any_order(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), None, D, 0, C.byref(plan)))
if shape == 'sbm10k_fused8':
    _hip.check(L.gemhip_gf_plan_set_fused_sweeps(plan, 8, 0))
info = (C.c_int64 * 8)(); _hip.check(L.gemhip_gf_plan_info(plan, info))
X = (0.01 * np.random.RandomState(1).randn(n, D)).astype(np.float32)
_hip.check(L.gemhip_gf_plan_set_embedding(plan, _hip.ptr(X, C.c_float)))
_hip.check(L.gemhip_gf_plan_sweeps(plan, 5, 1e-2, 1e-2, None))
_hip.check(L.gemhip_gf_plan_get_embedding(plan, _hip.ptr(X, C.c_float)))
digest = hashlib.sha256(X.tobytes()).hexdigest()
us = []
for rep in range(REPS + 1):                              # the first block warms up
    _hip.check(L.gemhip_synchronize(None))
    t0 = time.perf_counter()
    _hip.check(L.gemhip_gf_plan_sweeps(plan, sweeps, 1e-4, 1.0, None))
    _hip.check(L.gemhip_synchronize(None))
    us.append((time.perf_counter() - t0) / sweeps * 1e6)
_hip.check(L.gemhip_gf_plan_destroy(plan))
print(json.dumps(dict(shape=shape, lib=os.path.basename(_hip.LIB_PATH), sha256=digest, us_per_sweep=float(np.median(us[1:])), us_min=min(us[1:]), us_max=max(us[1:]),
                      updates=info[0], rows=info[1], levels=info[2], rows_per_wave=info[6], units=info[7])), flush=True)
