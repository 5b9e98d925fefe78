#!/usr/bin/env python3
"""Times the GPU t-SNE (gem_amd.evaluation.tsne.tsne_2d) on HOPE embeddings of SBM graphs.  A record, not a pass/fail bar: the capability is
new, there is no earlier time to compare with.

    python scripts/bench_tsne.py [--sizes 10000,100000,1000000] [--d 128] [--max-iter 1000] [--sklearn-upto 10000] [--out profiles/tsne.json]

Per size (nodes n, 10 n arcs, n / 1000 blocks, HOPE d = 128, beta = 0.01): the device time of the phases by HIP events (gemhip_tsne_last_ms:
kNN search, affinities, transpose, and the iterations summed over the calls), the milliseconds per iteration, the wall time of the whole
tsne_2d call, the final KL on the sparse P.  For sizes up to --sklearn-upto also the wall time of sklearn.manifold.TSNE (default barnes_hut) on
the same host and embedding, and the KL it reports.  Every size is a child process under its own `timeout`; the parent never opens the device and stops at the first
step that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def embedding(n, d):
    import numpy as np
    from gem_amd.embedding.hope import HOPE
    from gem_amd.graph import sbm_graph
    g = sbm_graph(n, 10 * n, max(n // 1000, 2), seed=1)
    t0 = time.perf_counter()
    X = HOPE(d=d, beta=0.01).learn_embedding(graph=g)
    return np.ascontiguousarray(X, dtype=np.float32), time.perf_counter() - t0


def step_gpu(a):
    from gem_amd.evaluation.tsne import tsne_2d
    X, embed_s = embedding(a.n, a.d)
    Y, info = tsne_2d(X, max_iter=a.max_iter)
    rec = {'n': a.n, 'arcs': 10 * a.n, 'd': a.d, 'hope_s': embed_s, 'max_iter': a.max_iter}
    rec.update({k: info[k] for k in ('k', 'n_iter', 'learning_rate', 'kl_divergence', 'knn_ms', 'affinity_ms', 'transpose_ms', 'iterations_ms', 'wall_s')})
    rec['ms_per_iteration'] = info['iterations_ms'] / max(info['n_iter'], 1)
    rec['pairs_per_s'] = float(a.n) * (a.n - 1) / (rec['ms_per_iteration'] * 1e-3)
    if a.sklearn:
        from sklearn.manifold import TSNE
        t0 = time.perf_counter()
        ref = TSNE(n_components=2, init='pca', random_state=0)
        ref.fit(X)
        rec['sklearn_barnes_hut_wall_s'] = time.perf_counter() - t0
        rec['sklearn_kl_divergence'] = float(ref.kl_divergence_)
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--sizes', default='10000,100000,1000000')
    p.add_argument('--d', type=int, default=128)
    p.add_argument('--max-iter', type=int, default=1000)
    p.add_argument('--sklearn-upto', type=int, default=10000)
    p.add_argument('--out', default=None)
    p.add_argument('--n', type=int, default=None, help='(child) one size')
    p.add_argument('--sklearn', type=int, default=0, help='(child) also time sklearn')
    p.add_argument('--step-timeout', type=int, default=900)
    a = p.parse_args()
    if a.n is not None:
        print('RESULT ' + json.dumps(step_gpu(a)), flush=True)
        return 0
    runs = []
    status = 0
    for n in [int(s) for s in a.sizes.split(',') if s]:
        cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--n', str(n), '--d', str(a.d), '--max-iter', str(a.max_iter),
               '--sklearn', str(int(n <= a.sklearn_upto))]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:])
            print('size %d failed with exit status %d: stopping' % (n, r.returncode))
            status = 1
            break
        runs.append(json.loads(line[-1][7:]))
        print(json.dumps(runs[-1]), flush=True)
    rec = {'what': 'tsne_2d on HOPE embeddings of SBM graphs, MI355X; times in ms are HIP events', 'runs': runs}
    if a.out and runs:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
