#!/usr/bin/env python3
"""Times the ranking metrics and link classification (gem_amd.evaluation.ranking / link_classification).  A record, not a pass/fail bar: the
capability is new, there is no earlier time to compare with.

    python scripts/bench_link_auc.py [--sort-sizes 20,24,26] [--graphs 100000,1000000] [--d 128] [--repeats 5] [--sklearn-upto 100000] [--out profiles/link_auc.json]

sort     per m = 2^k random fp64 scores and 0 / 1 labels: after a warm-up the median over --repeats calls of gemhip_rank_binary's kernel time
         (HIP events: keys, histograms, the passes, the scan, the terms) and of the call's wall time with host arrays in; keys per second;
         the bytes the kernels move per key by the count in DESIGN.md 3.5.5 (28 + 32 per pass for the sort, 69 for the metrics) and that
         rate against the 8 TB/s peak; on the same arrays numpy.argsort(kind='stable') and sklearn roc_auc_score + average_precision_score.
pairs    d = 128, m = 2^22 pairs (half arcs, half random) on the HOPE embedding of SBM 1M / 10M: the feature kernel and the fused score
         kernel (HIP events, medians), GB/s of their compulsory bytes (two rows read per pair, plus the feature row or the score written).
protocol per graph size n (SBM, 10 n arcs, 10 blocks; HOPE d = 128 on the train graph; Hadamard; an 80 / 20 split): sampling, the fit (passes x
         ms), scoring and ranking, AUC and AP; for n up to --sklearn-upto the same pairs through numpy float32 features and sklearn's
         LogisticRegression(solver='newton-cholesky', tol=1e-12) + roc_auc_score + average_precision_score on the host, the largest score
         deviation between the two and the share of (positive, negative) pairs within it: the bound on the AUC difference.
Every step is a child process under its own `timeout`; the parent never opens the device and stops at the first step that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_PEAK_TBS = 8.0
METRIC_BYTES_PER_KEY = 69           # flags 8 + 4 + 1 + 8, scan 8 + 8 + 8, groups 8 + 8 + 8 of the sorted keys, positions, labels and the packed scan


def step_sort(a):
    import numpy as np
    from gem_amd.evaluation import ranking as RK
    m = 1 << a.log2m
    rng = np.random.RandomState(a.log2m)
    y = (rng.random_sample(m) < 0.5).astype(np.uint8)
    s = rng.standard_normal(m) + 0.5 * y
    RK.binary_ranking_scores(s, y)
    kernel, wall = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        res = RK.binary_ranking_scores(s, y)
        wall.append(time.perf_counter() - t0)
        kernel.append(res['kernel_ms'])
    info = RK.sort_info()
    t0 = time.perf_counter()
    perm = RK.argsort_desc(s)
    argsort_wall = time.perf_counter() - t0
    kms = float(np.median(kernel))
    per_key = 28 + 32 * info['passes'] + METRIC_BYTES_PER_KEY
    rec = {'m': m, 'passes': info['passes'], 'kernel_ms': kms, 'kernel_ms_min': float(min(kernel)), 'kernel_ms_max': float(max(kernel)), 'wall_s': float(np.median(wall)), 'argsort_wall_s': argsort_wall, 'keys_per_s': m / (kms * 1e-3),
           'bytes_per_key': per_key, 'tb_per_s': per_key * m / (kms * 1e-3) / 1e12, 'share_of_hbm_peak': per_key * m / (kms * 1e-3) / 1e12 / HBM_PEAK_TBS,
           'auc': res['auc'], 'ap': res['ap'], 'n_thresholds': res['n_thresholds']}
    if a.sklearn:
        from sklearn.metrics import average_precision_score, roc_auc_score
        t0 = time.perf_counter()
        ref = np.argsort(-s, kind='stable')
        rec['numpy_argsort_s'] = time.perf_counter() - t0
        rec['perm_equal_numpy'] = bool(np.array_equal(ref, perm))
        t0 = time.perf_counter()
        auc = float(roc_auc_score(y, s)); ap = float(average_precision_score(y, s))
        rec['sklearn_auc_ap_s'] = time.perf_counter() - t0
        rec['sklearn_auc'] = auc; rec['sklearn_ap'] = ap
        rec['host_threads'] = int(os.environ.get('OMP_NUM_THREADS', '0'))
    else:
        rec['numpy_argsort_s'] = rec['sklearn_auc_ap_s'] = 'not run'
    return rec


def embed(n, d, graph):
    import numpy as np
    from gem_amd.embedding.hope import HOPE
    t0 = time.perf_counter()
    X = np.ascontiguousarray(HOPE(d=d, beta=0.01).learn_embedding(graph=graph), dtype=np.float32)
    return X, time.perf_counter() - t0


def step_pairs(a):
    import numpy as np
    from gem_amd.evaluation import link_classification as LC
    from gem_amd.graph import sbm_graph
    g = sbm_graph(a.n, 10 * a.n, 10, seed=1)
    X, hope_s = embed(a.n, a.d, g)
    m = 1 << 22
    rng = np.random.RandomState(0)
    pick = rng.randint(0, len(g.src), size=m // 2)
    st = np.concatenate([g.src[pick], rng.randint(0, a.n, size=m - m // 2)]).astype(np.int32)
    ed = np.concatenate([g.dst[pick], rng.randint(0, a.n, size=m - m // 2)]).astype(np.int32)
    w = rng.standard_normal(a.d + 1)
    rec = {'n': a.n, 'd': a.d, 'm': m, 'hope_s': hope_s}
    with LC.EdgeClassifier(X) as ec:
        ec.decision_function('hadamard', st, ed, w)
        sc, dt, ft = [], [], []
        for _ in range(a.repeats):
            ec.decision_function('hadamard', st, ed, w)
            sc.append(ec.stats()['scores_ms'])
            ec.dot(st, ed)
            dt.append(ec.stats()['scores_ms'])
        for _ in range(min(a.repeats, 3) + 1):                           # (the first is the warm-up; each call copies the 2 GiB matrix back)
            ec.features('hadamard', st, ed)
            ft.append(ec.stats()['features_ms'])
    row = 4.0 * a.d
    for name, ms, nbytes in (('scores', float(np.median(sc)), (2 * row + 8) * m), ('dot', float(np.median(dt)), (2 * row + 8) * m),
                             ('features', float(np.median(ft[1:])), 3 * row * m)):
        rec[name + '_kernel_ms'] = ms
        rec[name + '_compulsory_gb'] = nbytes / 1e9
        rec[name + '_gb_per_s'] = nbytes / 1e9 / (ms * 1e-3)
        rec[name + '_share_of_hbm_peak'] = nbytes / 1e12 / (ms * 1e-3) / HBM_PEAK_TBS
    rec['gather_amplification'] = 'not measured (no counter run was made)'
    return rec


def step_protocol(a):
    import numpy as np
    from gem_amd.evaluation import link_classification as LC
    from gem_amd.evaluation import ranking as RK
    from gem_amd.graph import sbm_graph
    from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
    g = sbm_graph(a.n, 10 * a.n, 10, seed=1)
    np.random.seed(0)
    t0 = time.perf_counter()
    train, test = split_di_graph_to_train_test(g, 0.8, True)
    split_s = time.perf_counter() - t0
    X, hope_s = embed(a.n, a.d, train)
    t0 = time.perf_counter()
    pairs = LC.link_pairs(train, test, seed=0)
    sample_s = time.perf_counter() - t0
    tst, ted, ty = pairs['test']
    with LC.EdgeClassifier(X) as ec:
        t0 = time.perf_counter()
        w, info = ec.fit('hadamard', *pairs['train'])
        fit_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        score = ec.decision_function('hadamard', tst, ted, w)
        score_s = time.perf_counter() - t0
        score_kernel_ms = ec.stats()['scores_ms']
        dot = ec.dot(tst, ted)
    t0 = time.perf_counter()
    res = RK.binary_ranking_scores(score, ty)
    rank_s = time.perf_counter() - t0
    res_dot = RK.binary_ranking_scores(dot, ty)
    rec = {'n': a.n, 'arcs': int(len(g.src)), 'd': a.d, 'op': 'hadamard', 'C': 1.0, 'split_s': split_s, 'hope_s': hope_s, 'sample_s': sample_s,
           'n_train_pairs': int(pairs['n_train_pos'] + pairs['n_train_neg']), 'n_test_pairs': int(pairs['n_test_pos'] + pairs['n_test_neg']), 'fit_s': fit_s,
           'fit_passes': info['passes'], 'fit_loss_evaluations': info['loss_evaluations'], 'fit_pass_ms': info['pass_ms'], 'fit_features_kernel_ms': info['fit_features_ms'],
           'fit_converged': bool(info['converged']), 'score_s': score_s, 'score_kernel_ms': score_kernel_ms, 'rank_s': rank_s, 'rank_kernel_ms': res['kernel_ms'],
           'auc': res['auc'], 'ap': res['ap'], 'auc_dot': res_dot['auc'], 'ap_dot': res_dot['ap']}
    if a.sklearn:
        import rank_refs as R
        from sklearn.linear_model import LogisticRegression
        from sklearn.metrics import average_precision_score, roc_auc_score
        st, ed, y = pairs['train']
        t0 = time.perf_counter()
        F = R.features_ref('hadamard', X, st, ed).astype(np.float64)
        model = LogisticRegression(C=1.0, solver='newton-cholesky', tol=1e-12, max_iter=1000).fit(F, y)
        rec['sklearn_fit_s'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        s_ref = model.decision_function(R.features_ref('hadamard', X, tst, ted).astype(np.float64))
        rec['sklearn_score_s'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        rec['sklearn_auc'] = float(roc_auc_score(ty, s_ref)); rec['sklearn_ap'] = float(average_precision_score(ty, s_ref))
        rec['sklearn_rank_s'] = time.perf_counter() - t0
        delta = float(np.abs(score - s_ref).max())
        rec['score_deviation'] = delta
        rec['near_share_at_deviation'] = R.near_pairs(s_ref, ty, 2 * delta) / float(pairs['n_test_pos'] * pairs['n_test_neg'])
        rec['auc_difference'] = abs(rec['auc'] - rec['sklearn_auc']); rec['ap_difference'] = abs(rec['ap'] - rec['sklearn_ap'])
        rec['coef_deviation'] = float(np.abs(w - np.append(model.coef_[0], model.intercept_[0])).max() / np.abs(model.coef_).max())
        rec['host_threads'] = int(os.environ.get('OMP_NUM_THREADS', '0'))
    else:
        rec['sklearn_fit_s'] = 'not run'
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--sort-sizes', default='20,24,26')
    p.add_argument('--graphs', default='100000,1000000')
    p.add_argument('--pairs-n', type=int, default=1000000)
    p.add_argument('--d', type=int, default=128)
    p.add_argument('--repeats', type=int, default=5)
    p.add_argument('--sklearn-upto', type=int, default=100000)
    p.add_argument('--sort-sklearn-upto', type=int, default=26)
    p.add_argument('--out', default=None)
    p.add_argument('--step', default=None, help='(child) sort, pairs or protocol')
    p.add_argument('--log2m', type=int, default=None, help='(child)')
    p.add_argument('--n', type=int, default=None, help='(child)')
    p.add_argument('--sklearn', type=int, default=0, help='(child) also time the host baseline')
    p.add_argument('--step-timeout', type=int, default=300)
    a = p.parse_args()
    if a.step:
        print('RESULT ' + json.dumps({'sort': step_sort, 'pairs': step_pairs, 'protocol': step_protocol}[a.step](a)), flush=True)
        return 0
    env = dict(os.environ)
    env.setdefault('OMP_NUM_THREADS', '16')
    steps = [('sort', ['--log2m', k, '--sklearn', str(int(int(k) <= a.sort_sklearn_upto))]) for k in a.sort_sizes.split(',') if k]
    if a.pairs_n:
        steps.append(('pairs', ['--n', str(a.pairs_n)]))
    steps += [('protocol', ['--n', n, '--sklearn', str(int(int(n) <= a.sklearn_upto))]) for n in a.graphs.split(',') if n]
    rec = {'what': 'ranking metrics and link classification on one MI355X; *_kernel_ms are HIP events, medians of %d runs after a warm-up; *_s host wall; '
                   'rates against the %g TB/s HBM peak' % (a.repeats, HBM_PEAK_TBS), 'sort': [], 'pairs': [], 'protocol': []}
    status = 0
    for step, extra in steps:
        cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--step', step, '--d', str(a.d), '--repeats', str(a.repeats)] + extra
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:])
            print('step %s %s failed with exit status %d: stopping' % (step, ' '.join(extra), r.returncode))
            status = 1
            break
        rec[step].append(json.loads(line[-1][7:]))
        print(step, json.dumps(rec[step][-1]), flush=True)
    if a.out and (rec['sort'] or rec['pairs'] or rec['protocol']):
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
