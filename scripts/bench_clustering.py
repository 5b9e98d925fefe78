#!/usr/bin/env python3
"""Times k-means (gem_amd.evaluation.clustering) on HOPE embeddings of SBM graphs with the blocks as clusters.  A record, not a pass/fail
bar: the capability is new, there is no earlier time to compare with.

    python scripts/bench_clustering.py [--sizes 10000:10,100000:32,1000000:100] [--d 128] [--repeats 5] [--sklearn-upto 1000000] [--out profiles/clustering.json]

Per size n:B (nodes n, 10 n arcs, B blocks = B clusters, HOPE d = 128, beta = 0.01): the upload, the k-means++ seeding (host wall), and after
one warm-up fit the median over --repeats fits from the same seeded centres of the fit time (HIP events around the iterations) and of
that over the iteration count; the assign kernel alone (HIP events, median of --repeats calls) against its two floors -- 2 n K d flop at the
122 TF/s an untuned fp32-MFMA GEMM reaches, and one read of X at 5 TB/s --; the update step alone; NMI and ARI against the blocks.  For
comparison sklearn.cluster.KMeans(algorithm='lloyd', init=<the same centres>, n_init=1, max_iter=<the same iteration count>, tol=0) on the
same host, 16 threads, for sizes up to --sklearn-upto.  Every size is a child process under its own `timeout`; the parent never opens the
device and stops at the first step that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_GEMM_TFLOPS = 122.0
HBM_TBS = 5.0


def step_gpu(a):
    import numpy as np
    from gem_amd.embedding.hope import HOPE
    from gem_amd.evaluation import clustering as CL
    from gem_amd.graph import sbm_block_labels, sbm_graph
    g = sbm_graph(a.n, 10 * a.n, a.blocks, seed=1)
    t0 = time.perf_counter()
    X = np.ascontiguousarray(HOPE(d=a.d, beta=0.01).learn_embedding(graph=g), dtype=np.float32)
    hope_s = time.perf_counter() - t0
    y = sbm_block_labels(a.n, a.blocks).astype(np.int32)
    K = a.blocks
    with CL.KMeans(X) as km:
        _, C0 = km.seed_pp(K, seed=0)
        seed_ms = km.stats()['seed_ms']
        km.fit(K, init=C0, warn=False)                                   # warm-up
        fits = []
        for _ in range(a.repeats):
            labels, C, info = km.fit(K, init=C0, warn=False)
            fits.append((info['fit_ms'], info['iteration_ms']))
        table = km.contingency(y, K)
        assign = []
        for _ in range(a.repeats):
            km.assign(K, C)
            assign.append(km.stats()['assign_ms'])
        km.update(K, labels)
        update = []
        for _ in range(a.repeats):
            km.update(K, labels)
            update.append(km.stats()['update_ms'])
        st = km.stats()
    nmi, ari, purity, _ = CL.clustering_scores(table)
    assign_ms = float(np.median(assign))
    flop = 2.0 * a.n * K * a.d
    floor_flop_ms = flop / (F32_GEMM_TFLOPS * 1e12) * 1e3
    floor_byte_ms = 4.0 * a.n * st['d_padded'] / (HBM_TBS * 1e12) * 1e3
    rec = {'n': a.n, 'arcs': 10 * a.n, 'd': a.d, 'K': K, 'hope_s': hope_s, 'upload_ms': st['upload_ms'], 'seed_ms': seed_ms,
           'iterations': info['iterations'], 'strict': bool(info['strict']), 'converged': bool(info['converged']), 'relocations': info['relocations'],
           'fit_ms': float(np.median([f[0] for f in fits])), 'ms_per_iteration': float(np.median([f[1] for f in fits])), 'assign_kernel_ms': assign_ms,
           'update_ms': float(np.median(update)), 'assign_flop': flop, 'assign_tflops': flop / (assign_ms * 1e-3) / 1e12,
           'assign_flop_floor_ms': floor_flop_ms, 'assign_byte_floor_ms': floor_byte_ms, 'assign_share_of_flop_floor': floor_flop_ms / assign_ms,
           'assign_share_of_byte_floor': floor_byte_ms / assign_ms, 'inertia': info['inertia'], 'nmi': nmi, 'ari': ari, 'purity': purity}
    if a.sklearn:
        from sklearn.cluster import KMeans
        from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
        import warnings
        X64 = X.astype(np.float64)
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            sk = KMeans(n_clusters=K, init=C0.astype(np.float64), n_init=1, algorithm='lloyd', tol=0.0, max_iter=info['iterations']).fit(X64)
        rec['sklearn_fit_wall_s'] = time.perf_counter() - t0
        rec['sklearn_iterations'] = int(sk.n_iter_)
        rec['sklearn_ms_per_iteration'] = rec['sklearn_fit_wall_s'] * 1e3 / max(int(sk.n_iter_), 1)
        rec['sklearn_nmi'] = float(normalized_mutual_info_score(y, sk.labels_)); rec['sklearn_ari'] = float(adjusted_rand_score(y, sk.labels_))
        rec['sklearn_threads'] = int(os.environ.get('OMP_NUM_THREADS', '0'))
        rec['labels_equal_sklearn'] = bool(np.array_equal(sk.labels_, labels))
    else:
        rec['sklearn_fit_wall_s'] = 'not run'
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--sizes', default='10000:10,100000:32,1000000:100')
    p.add_argument('--d', type=int, default=128)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--sklearn-upto', type=int, default=1000000)
    p.add_argument('--out', default=None)
    p.add_argument('--n', type=int, default=None, help='(child) one size')
    p.add_argument('--blocks', type=int, default=None, help='(child) its blocks')
    p.add_argument('--sklearn', type=int, default=0, help='(child) also time sklearn')
    p.add_argument('--step-timeout', type=int, default=420)
    a = p.parse_args()
    if a.n is not None:
        print('RESULT ' + json.dumps(step_gpu(a)), flush=True)
        return 0
    runs = []
    status = 0
    env = dict(os.environ)
    env.setdefault('OMP_NUM_THREADS', '16')
    for n, blocks in [tuple(int(v) for v in s.split(':')) for s in a.sizes.split(',') if s]:
        cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--n', str(n), '--blocks', str(blocks), '--d', str(a.d),
               '--repeats', str(a.repeats), '--sklearn', str(int(n <= a.sklearn_upto))]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:])
            print('size %d failed with exit status %d: stopping' % (n, r.returncode))
            status = 1
            break
        runs.append(json.loads(line[-1][7:]))
        print(json.dumps(runs[-1]), flush=True)
    rec = {'what': 'k-means on HOPE embeddings of SBM graphs, MI355X; fit_ms, ms_per_iteration, assign_kernel_ms and update_ms are HIP events, medians of '
                   '%d runs after a warm-up; seed_ms and upload_ms host wall; floors: 2 n K d flop at %g TF/s, one read of X at %g TB/s' % (a.repeats, F32_GEMM_TFLOPS,
                                                                                                                                    HBM_TBS), 'runs': runs}
    if a.out and runs:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
