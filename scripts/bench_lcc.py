#!/usr/bin/env python3
"""Times the largest-connected-component step (gemhip_lcc, gem_amd/csrc/cc.hip) against the host path it replaces.  A record, not a pass/fail bar.

    python scripts/bench_lcc.py [--graphs sbm1m,rmat20,rmat22] [--reps 7] [--out profiles/lcc.json]

Graphs: SBM 1M nodes / 10M arcs (the benchmark graph's shape), R-MAT scale 20 / 16M arcs, R-MAT scale 22 / 64M arcs.  Per graph, after one
warm-up call, `reps` repetitions of each side; every list of repetitions is kept, the figures quoted are medians with min and max beside them:
  gpu.wall_s          gem_amd.graph.lcc_arrays: host arrays in, host arrays out (ctypes call, validation, uploads, kernels, copies back)
  gpu.phases          gemhip_last_call_phases of the same calls (host validation, h2d, kernels by HIP events, d2h), medians
  gpu.kernel_ms       gemhip_cc_last_kernel_ms: init, union, flatten, sizes, winner, node compaction, arc compaction, medians
  host.wall_s         the same result on this machine's CPU: scipy CSR build + connected_components(connection='weak') + numpy compaction
                      (bincount, argmax, flatnonzero, boolean masks), split into its three steps
  speedup             host.wall_s / gpu.wall_s (medians)
The two sides are checked to agree (node and arc counts, component count, the arrays themselves) before anything is recorded.
Every graph is a child process under its own `timeout`; the parent never opens the device and stops at the first child that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ('init', 'union', 'flatten', 'sizes', 'winner', 'compact_nodes', 'compact_arcs')
GRAPHS = {'sbm1m': ('sbm', 1000000, 10000000), 'rmat20': ('rmat', 20, 16000000), 'rmat22': ('rmat', 22, 64000000),
          'rmat14': ('rmat', 14, 65536)}            # (rmat14: the test suite's graph, for a quick look)


def spread(xs):
    import numpy as np
    return {'median': float(np.median(xs)), 'min': float(min(xs)), 'max': float(max(xs)), 'all': [float(x) for x in xs]}


def host_lcc(n, src, dst):
    """The host path, timed step by step: (results, seconds of csr build, connected_components, compaction)."""
    import numpy as np
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    A = sp.csr_matrix((np.ones(len(src), dtype=np.int8), (src, dst)), shape=(n, n))
    t1 = time.perf_counter()
    ncomp, lab = connected_components(A, directed=True, connection='weak')
    t2 = time.perf_counter()
    size = np.bincount(lab, minlength=ncomp)
    first = np.full(ncomp, n, dtype=np.int64)
    first[lab[::-1]] = np.arange(n - 1, -1, -1)                       # smallest node id of every component
    big = np.flatnonzero(size == size.max())
    winner = big[np.argmin(first[big])]
    keep = lab == winner
    old_of_new = np.flatnonzero(keep).astype(np.int32)
    new_of_old = np.full(n, -1, dtype=np.int32)
    new_of_old[old_of_new] = np.arange(len(old_of_new), dtype=np.int32)
    ka = keep[src]
    s, d = new_of_old[src[ka]], new_of_old[dst[ka]]
    t3 = time.perf_counter()
    return (int(ncomp), old_of_new, new_of_old, s, d), (t1 - t0, t2 - t1, t3 - t2)


def child(name, reps):
    import ctypes as C
    import numpy as np
    from gem_amd import _hip
    from gem_amd.graph import lcc_arrays, rmat_graph, sbm_graph
    kind, a, arcs = GRAPHS[name]
    g = sbm_graph(a, arcs, 100, seed=20260927) if kind == 'sbm' else rmat_graph(a, arcs, 5)
    n, src, dst = g.n, g.src, g.dst
    ref, _ = host_lcc(n, src, dst)
    got = lcc_arrays(n, src, dst)                                     # warm-up: device, library, first-touch of the buffers
    assert got[0] == ref[0] and all(np.array_equal(x, y) for x, y in zip(got[1:5], ref[1:])), 'device and host disagree'
    wall, phases, kms = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        lcc_arrays(n, src, dst)
        wall.append(time.perf_counter() - t0)
        phases.append(_hip.last_call_phases())
        out = (C.c_double * 8)()
        _hip.check(_hip.lib().gemhip_cc_last_kernel_ms(out))
        kms.append(list(out)[:len(KERNELS)])
    host = [host_lcc(n, src, dst)[1] for _ in range(max(3, reps // 2))]
    host_wall = [sum(h) for h in host]
    rec = {'graph': {'kind': kind, 'n': int(n), 'arcs': int(len(src)), 'n_components': ref[0], 'lcc_nodes': int(len(ref[1])), 'lcc_arcs': int(len(ref[3]))},
           'gpu': {'wall_s': spread(wall),
                   'phases': {k: float(np.median([p[k] for p in phases])) for k in phases[0]},
                   'kernel_ms': {k: spread([r[i] for r in kms]) for i, k in enumerate(KERNELS)}},
           'host': {'wall_s': spread(host_wall), 'csr_build_s': spread([h[0] for h in host]), 'connected_components_s': spread([h[1] for h in host]),
                    'compaction_s': spread([h[2] for h in host])}}
    rec['speedup'] = rec['host']['wall_s']['median'] / rec['gpu']['wall_s']['median']
    km = rec['gpu']['kernel_ms']
    rec['gpu']['slowest_kernel'] = max(KERNELS, key=lambda k: km[k]['median'])
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', default='sbm1m,rmat20,rmat22')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lcc.json'))
    ap.add_argument('--timeout', type=int, default=420, help='seconds per graph')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps)
        return 0
    result = {'what': 'gemhip_lcc vs scipy connected_components + numpy compaction on the same machine (scripts/bench_lcc.py)', 'reps': a.reps,
              'graphs': {}}
    for name in a.graphs.split(','):
        r = subprocess.run(['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', name, '--reps', str(a.reps)],
                           stdout=subprocess.PIPE, universal_newlines=True)
        if r.returncode != 0:
            print('bench_lcc: %s ended with status %d; stopping' % (name, r.returncode), file=sys.stderr)
            return 1
        result['graphs'][name] = json.loads(r.stdout.strip().splitlines()[-1])
        rec = result['graphs'][name]
        print('%-7s gpu %.1f ms  host %.1f ms  x%.1f  kernels %.2f ms (slowest: %s)' % (
            name, 1e3 * rec['gpu']['wall_s']['median'], 1e3 * rec['host']['wall_s']['median'], rec['speedup'], 1e3 * rec['gpu']['phases']['kernels_s'],
            rec['gpu']['slowest_kernel']), flush=True)
        with open(a.out, 'w') as fh:
            json.dump(result, fh, indent=1)
            fh.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
