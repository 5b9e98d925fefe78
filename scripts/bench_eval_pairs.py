#!/usr/bin/env python3
"""Times the pair-sampled GPU evaluator (gemhip_eval_pairs, evaluate_reconstruction_gpu) at scale.  A record, not a pass/fail bar.

    python scripts/bench_eval_pairs.py [--n 1000000] [--d 128] [--ratio 1e-5] [--out profiles/eval_pairs.json]

Default shape: n = 1M nodes, d = 128, ratio 1e-5 undirected = 4 999 995 random pairs, random X, an SBM graph of 16M arcs.  Reported:
  kernel_ms          the pair kernel alone, by HIP events (gemhip_eval_last_pairs_ms), median of 5 launches after one warm-up
  pairs_per_s        pairs / kernel time
  gather_TBps        pairs * (2*4*d + 8) B / kernel time -- two rows and two indices per pair; next to it the ~6.3 TB/s a streaming
                     read achieves on MI355X HBM3E (8 TB/s peak) and the 5.5-5.8 TB/s measured for random whole-row gathers of >= 1 KiB rows
  call_s             one whole evaluate_reconstruction_gpu(edge_pairs=...) call: CSR build, uploads, kernel, copies back, host metrics
  host_sort_s        pair_metrics alone on the call's scores (the two stable sorts and the group arithmetic)
Every GPU step is a child process under its own `timeout`; the parent never opens the device and stops at the first step that fails."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_ACHIEVABLE_TBPS = 6.3


def problem(a):
    import numpy as np
    from gem_amd.evaluation import reconstruction as gr
    from gem_amd.graph import sbm_graph
    g = sbm_graph(a.n, a.arcs, max(a.n // 1024, 1), seed=1)
    X = np.random.default_rng(0).standard_normal((a.n, a.d), dtype=np.float32) * np.float32(0.1)
    pairs = gr.random_edge_pairs(a.n, a.ratio, True, seed=0)
    return g, X, pairs


def step_kernel(a):
    import numpy as np
    from gem_amd.evaluation import reconstruction as gr
    g, X, pairs = problem(a)
    st, ed = gr._pair_arrays(pairs)
    ms = []
    with gr._DeviceEvaluator(g.n, g.src, g.dst, None, X) as ev:
        for _ in range(6):
            ev.pairs(st, ed)
            ms.append(ev.last_pairs_ms())
    k = float(np.median(ms[1:]))
    m = len(st)
    return {'pairs': m, 'kernel_ms': k, 'kernel_ms_all': ms, 'pairs_per_s': m / (k * 1e-3),
            'gather_TBps': m * (2 * 4 * a.d + 8) / (k * 1e-3) / 1e12, 'hbm_achievable_TBps': HBM_ACHIEVABLE_TBPS}


def step_call(a):
    from gem_amd.evaluation import reconstruction as gr
    g, X, pairs = problem(a)
    gr.evaluate_reconstruction_gpu(g, None, X, edge_pairs=pairs[:1000])                      # device and library warm
    t0 = time.perf_counter()
    MAP, prec, _, _ = gr.evaluate_reconstruction_gpu(g, None, X, edge_pairs=pairs)
    call = time.perf_counter() - t0
    st, ed = gr._pair_arrays(pairs)
    with gr._DeviceEvaluator(g.n, g.src, g.dst, None, X) as ev:
        score, hit = ev.pairs(st, ed)
    t0 = time.perf_counter()
    MAP2, _ = gr.pair_metrics(g.n, st, ed, score, hit, True)
    sort = time.perf_counter() - t0
    assert MAP2 == MAP
    return {'call_s': call, 'host_sort_s': sort, 'host_sort_share': sort / call, 'MAP': MAP, 'curve_len': len(prec)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000000)
    p.add_argument('--d', type=int, default=128)
    p.add_argument('--ratio', type=float, default=1e-5)
    p.add_argument('--arcs', type=int, default=16000000)
    p.add_argument('--out', default=None)
    p.add_argument('--step', choices=('kernel', 'call'), default=None)
    p.add_argument('--step-timeout', type=int, default=240)
    a = p.parse_args()
    if a.step:
        print('RESULT ' + json.dumps({'kernel': step_kernel, 'call': step_call}[a.step](a)), flush=True)
        return 0
    rec = {'n': a.n, 'd': a.d, 'ratio': a.ratio, 'arcs': a.arcs}
    for step in ('kernel', 'call'):
        cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--step', step, '--n', str(a.n), '--d', str(a.d),
               '--ratio', repr(a.ratio), '--arcs', str(a.arcs)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            print(r.stdout[-2000:])
            print('step %s failed with exit status %d: stopping' % (step, r.returncode))
            return 1
        rec.update(json.loads(line[-1][7:]))
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == '__main__':
    sys.exit(main())
