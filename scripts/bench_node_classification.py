#!/usr/bin/env python3
"""Times node classification (gem_amd.evaluation.node_classification) on HOPE embeddings of SBM graphs with their block labels.  A record, not
a pass/fail bar: the capability is new, there is no earlier time to compare with.

    python scripts/bench_node_classification.py [--sizes 10000:10,100000:32,1000000:100] [--d 128] [--sklearn-upto 10000] [--out profiles/node_classification.json]

Per size n:B (nodes n, 10 n arcs, B blocks = B classes, HOPE d = 128, beta = 0.01, 30 % test rows, seed 0, C = 1): the upload and fit wall
time, the Newton passes and the mean milliseconds per pass (host wall around the pass kernels, their reduction and the copy back of F, g, H),
the rate of the pass's Hessian work -- n_train * K * upper-triangle tiles * 2048 flop -- against the 157.3 TF/s f32 matrix peak, the predict
time (HIP events) and the three metrics.  For sizes up to --sklearn-upto also the wall time of
OneVsRestClassifier(LogisticRegression()).fit + decision_function on the same host, and its metrics under the same top-k ranker; larger
sizes are marked "not run".  Every size is a child process under its own `timeout`; the parent never opens the device and stops at the
first step that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_MATRIX_PEAK_TFLOPS = 157.3


def step_gpu(a):
    import numpy as np
    from gem_amd.embedding.hope import HOPE
    from gem_amd.evaluation import node_classification as NC
    from gem_amd.graph import sbm_block_labels, sbm_graph
    g = sbm_graph(a.n, 10 * a.n, a.blocks, seed=1)
    t0 = time.perf_counter()
    X = np.ascontiguousarray(HOPE(d=a.d, beta=0.01).learn_embedding(graph=g), dtype=np.float32)
    hope_s = time.perf_counter() - t0
    y = sbm_block_labels(a.n, a.blocks)
    train, test = NC.split_nodes(a.n, 0.3, 0)
    t0 = time.perf_counter()
    with NC.NodeClassifier(X) as nc:
        nc.set_labels(y)
        _, _, info = nc.fit(train)
        _, tp, fp, fn, exact = nc.predict_topk(test, want_pred=False)
        st = nc.stats()
    wall_s = time.perf_counter() - t0
    micro, macro = NC.f1_from_counts(tp, fp, fn)
    T = (a.d + 1 + 31) // 32
    flop = float(len(train)) * a.blocks * (T * (T + 1) // 2) * 2048
    rec = {'n': a.n, 'arcs': 10 * a.n, 'd': a.d, 'K': a.blocks, 'n_train': int(len(train)), 'n_test': int(len(test)), 'hope_s': hope_s, 'wall_s': wall_s,
           'upload_ms': st['upload_ms'], 'fit_ms': st['fit_ms'], 'newton_passes': st['passes'], 'loss_evaluations': st['loss_evaluations'],
           'ms_per_pass': st['pass_ms'], 'pass_hessian_flop': flop, 'pass_tflops': flop / (st['pass_ms'] * 1e-3) / 1e12,
           'pass_share_of_f32_matrix_peak': flop / (st['pass_ms'] * 1e-3) / 1e12 / F32_MATRIX_PEAK_TFLOPS, 'predict_ms': st['predict_ms'],
           'converged': bool(info['converged'].all()), 'iterations_max': int(info['iterations'].max()), 'backtracks': int(info['backtracks'].sum()),
           'micro_f1': micro, 'macro_f1': macro, 'accuracy': exact / float(len(test))}
    if a.sklearn:
        from sklearn.linear_model import LogisticRegression
        from sklearn.multiclass import OneVsRestClassifier
        Y = np.zeros((a.n, a.blocks), np.uint8); Y[np.arange(a.n), y] = 1
        t0 = time.perf_counter()
        ovr = OneVsRestClassifier(LogisticRegression()).fit(X[train].astype(np.float64), Y[train])
        S = ovr.decision_function(X[test].astype(np.float64))
        rec['sklearn_fit_predict_wall_s'] = time.perf_counter() - t0
        pred = np.zeros_like(Y[test]); pred[np.arange(len(test)), np.argmax(S, axis=1)] = 1          # one label per node: top-1
        tp = (pred & Y[test]).sum(0); fp = (pred & ~Y[test] & 1).sum(0); fn = (~pred & 1 & Y[test]).sum(0)
        rec['sklearn_micro_f1'], rec['sklearn_macro_f1'] = NC.f1_from_counts(tp, fp, fn)
    else:
        rec['sklearn_fit_predict_wall_s'] = 'not run'
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--sizes', default='10000:10,100000:32,1000000:100')
    p.add_argument('--d', type=int, default=128)
    p.add_argument('--sklearn-upto', type=int, default=10000)
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
    for n, blocks in [tuple(int(v) for v in s.split(':')) for s in a.sizes.split(',') if s]:
        cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--n', str(n), '--blocks', str(blocks), '--d', str(a.d),
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
    rec = {'what': 'node classification on HOPE embeddings of SBM graphs, MI355X; ms_per_pass and fit_ms are host wall, predict_ms HIP events', 'runs': runs}
    if a.out and runs:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
