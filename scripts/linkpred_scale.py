#!/usr/bin/env python3
"""Link prediction at scale: device times of the masked AP stream and the per-node top-k next to the unmasked AP kernel.  A record, not a bar.

    python scripts/linkpred_scale.py [--n 1000000] [--arcs 10000000] [--d 128] [--nodes 4096] [--k 100] [--out profiles/linkpred_eval.json]

Workload: an SBM graph (default 1M nodes / 10M arcs), split_di_graph_to_train_test at 0.8 (undirected, np.random.seed(--seed)), GF trained on
the TRAIN graph, `--nodes` nodes from eligible_sample of the TEST graph.  On ONE evaluator handle (test CSR + trained table, train graph as
mask), after one warm-up round, three rounds of
  ap_ms          gemhip_eval_ap          eval_ap_kernel<NV, KIND, false>, the unmasked stream: the baseline
  ap_masked_ms   gemhip_eval_ap_masked   eval_ap_kernel<NV, KIND, true>: the same rows plus a walk through one mask row per node
  topk_ms        gemhip_eval_topk        eval_topk_kernel at k = --k
each a HIP-event time of the kernel alone (gemhip_eval_last_kernel_ms).  `masked_over_ap` is the ratio of the medians, `ap_spread` and
`ap_masked_spread` are (max - min) / median of the three repeats.  Also recorded: the link-prediction MAP (mean masked AP of the sample) of the
trained table and of GF's untrained initial table 0.01 * RandomState(seed).randn (gf.py:92), the reconstruction-style MAP of the same nodes
without the mask, and the mean precision@k.
The measurement is a child process under its own `timeout`; the parent never opens the device."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(a):
    import numpy as np
    from gem_amd.embedding.gf import GraphFactorization
    from gem_amd.evaluation import reconstruction as gr
    from gem_amd.graph import sbm_graph
    from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
    def say(what):
        print('[linkpred_scale] %s' % what, file=sys.stderr, flush=True)
    t0 = time.perf_counter()
    g = sbm_graph(a.n, a.arcs, max(a.n // 10000, 1), seed=1)
    np.random.seed(a.seed)
    train, test = split_di_graph_to_train_test(g, 0.8, is_undirected=True)
    t_split = time.perf_counter()
    say('graph and split: %.1f s, %d train arcs, %d test arcs' % (t_split - t0, len(train.src), len(test.src)))
    model = GraphFactorization(d=a.d, eta=a.eta, regu=a.regu, max_iter=a.max_iter, seed=a.seed, device_init=False)
    X = model.learn_embedding(graph=train)
    t_train = time.perf_counter()
    say('GF trained: %.1f s' % (t_train - t_split))
    X0 = (0.01 * np.random.RandomState(a.seed).randn(a.n, a.d)).astype(np.float32)          # the table that training started from
    nodes = gr.eligible_sample(test, a.nodes)
    rec = {'train_arcs': int(len(train.src)), 'test_arcs': int(len(test.src)), 'sampled_nodes': int(len(nodes)),
           'host_s': {'graph_and_split': t_split - t0, 'gf_learn_embedding': t_train - t_split}}
    times = {'ap_ms': [], 'ap_masked_ms': [], 'topk_ms': []}
    with gr._DeviceEvaluator(test.n, test.src, test.dst, model, X) as ev:
        ev.set_mask(train.src, train.dst)
        for rep in range(4):                                          # round 0 warms up
            plain = ev.ap(nodes, True); t_ap = ev.last_kernel_ms()
            (ap, npos) = ev.ap_masked(nodes, True); t_m = ev.last_kernel_ms()
            ids, score, hit = ev.topk(nodes, a.k, True); t_k = ev.last_kernel_ms()
            say('round %d: ap %.1f ms, ap_masked %.1f ms, topk %.1f ms' % (rep, t_ap, t_m, t_k))
            if rep:
                times['ap_ms'].append(t_ap); times['ap_masked_ms'].append(t_m); times['topk_ms'].append(t_k)
        rec.update({'MAP_linkpred_trained': float(ap.mean()), 'MAP_unmasked_trained': float(plain.mean()), 'positives_ranked': int(npos.sum()),
                    'precision_at_k_trained': float(hit.sum(axis=1).mean() / a.k), 'short_lists': int((ids[:, -1] < 0).sum())})
    with gr._DeviceEvaluator(test.n, test.src, test.dst, model, X0) as ev:
        ev.set_mask(train.src, train.dst)
        rec['MAP_linkpred_untrained'] = float(ev.ap_masked(nodes, True)[0].mean())
    med = {k: float(np.median(v)) for k, v in times.items()}
    rec.update(times)
    rec.update({'ap_ms_median': med['ap_ms'], 'ap_masked_ms_median': med['ap_masked_ms'], 'topk_ms_median': med['topk_ms'],
                'masked_over_ap': med['ap_masked_ms'] / med['ap_ms'], 'topk_over_ap': med['topk_ms'] / med['ap_ms'],
                'ap_spread': (max(times['ap_ms']) - min(times['ap_ms'])) / med['ap_ms'],
                'ap_masked_spread': (max(times['ap_masked_ms']) - min(times['ap_masked_ms'])) / med['ap_masked_ms']})
    return rec


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=1000000)
    p.add_argument('--arcs', type=int, default=10000000)
    p.add_argument('--d', type=int, default=128)
    p.add_argument('--nodes', type=int, default=4096)
    p.add_argument('--k', type=int, default=100)
    p.add_argument('--eta', type=float, default=0.01)
    p.add_argument('--regu', type=float, default=0.01)
    p.add_argument('--max-iter', type=int, default=100)
    p.add_argument('--seed', type=int, default=5)
    p.add_argument('--out', default=None)
    p.add_argument('--child', action='store_true')
    p.add_argument('--step-timeout', type=int, default=900)
    a = p.parse_args()
    if a.child:
        print('RESULT ' + json.dumps(measure(a)), flush=True)
        return 0
    rec = {'n': a.n, 'arcs': a.arcs, 'd': a.d, 'k': a.k, 'train_ratio': 0.8, 'gf': {'eta': a.eta, 'regu': a.regu, 'max_iter': a.max_iter, 'seed': a.seed}}
    cmd = ['timeout', '-k', '10', str(a.step_timeout), sys.executable, os.path.abspath(__file__), '--child', '--n', str(a.n), '--arcs', str(a.arcs),
           '--d', str(a.d), '--nodes', str(a.nodes), '--k', str(a.k), '--eta', repr(a.eta), '--regu', repr(a.regu), '--max-iter', str(a.max_iter),
           '--seed', str(a.seed)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)          # the child's progress lines go to stderr as they come
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    if r.returncode != 0 or not line:
        print(r.stdout[-2000:])
        print('the measurement failed with exit status %d' % r.returncode)
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
