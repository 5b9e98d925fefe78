"""Measures the neighbourhood link-prediction scores (gem_amd/csrc/nbr.hip) on an MI355X and writes profiles/link_baselines.json.

    python scripts/bench_link_baselines.py [--rows sbm1m,rmat20,rmat22] [--repeats 5] [--ab-libs name=path,...] [--ab-rows sbm1m,rmat20]

Rows
  sbm1m    sbm_graph(1M nodes, 10M arcs, 100 blocks), split 80 / 20 on numpy seed 0, link_pairs(seed 0): ALL test pairs scored on the train graph.
  rmat20   rmat_graph(20, 16M arcs): 1M arcs of the graph (adjacent pairs, hub-heavy: an arc's endpoints are drawn by degree) and 1M uniform
  rmat22   rmat_graph(22, 64M arcs)  pairs u != v, scored on the whole graph.
Per row: host ingest and graph upload, and per call the plan (host wall), the pair and item upload, the kernels (HIP events, median and range
over --repeats calls after one warm-up) and the download; the end-to-end wall time of scores(); pairs / s by kernel time and end to end; the
item counts per class and the longest item.  The comparator is the scipy row product of tests/nbr_refs.py on the first 100 000 pairs of a
fixed shuffle, on the same host, single process.

Every measurement runs in a child process of its own (a library is loaded once per process); the parent never opens the device.  --ab-libs
names further builds of the library with other constants (GEM_HIP_EXTRA_CFLAGS=-DGEMHIP_NBR_CHUNK=... python -m gem_amd.build, copied
aside); they are run alternately with the tree's library, --ab-rounds times each, on --ab-rows, and must return the same cn."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
SAMPLE = 100000


def make_row(name):
    """(graph, st, ed, what): host only."""
    import numpy as np
    from gem_amd.graph import rmat_graph, sbm_graph
    if name in ('sbm1m', 'sbm10k'):                                   # (sbm10k: a rehearsal size, not a row of the profile)
        from gem_amd.evaluation.link_classification import link_pairs
        from gem_amd.utils.evaluation_util import split_di_graph_to_train_test
        g = sbm_graph(1000000, 10000000, 100, seed=20260927) if name == 'sbm1m' else sbm_graph(10000, 100000, 10, seed=1)
        np.random.seed(0)
        train, test = split_di_graph_to_train_test(g, 0.8, True)
        t0 = time.perf_counter()
        pairs = link_pairs(train, test, seed=0)
        return train, pairs['test'][0], pairs['test'][1], {'graph': 'sbm_graph(1000000, 10000000, 100), 80 / 20 split', 'pairs': 'all test pairs of link_pairs(seed=0)',
                                                           'n_test_pos': int(pairs['n_test_pos']), 'n_test_neg': int(pairs['n_test_neg']),
                                                           'link_pairs_s': time.perf_counter() - t0}
    scale, arcs = {'rmat20': (20, 16 << 20), 'rmat22': (22, 64 << 20)}[name]
    g = rmat_graph(scale, arcs, 5)
    rng = np.random.RandomState(0)
    half = 1 << 20
    pick = rng.randint(0, len(g.src), size=half)
    u = rng.randint(0, g.n, size=half); v = rng.randint(0, g.n, size=half)
    v = np.where(u == v, (v + 1) % g.n, v)
    st = np.concatenate([g.src[pick], u]).astype(np.int32); ed = np.concatenate([g.dst[pick], v]).astype(np.int32)
    return g, st, ed, {'graph': 'rmat_graph(%d, %d, 5)' % (scale, arcs), 'pairs': '%d arcs of the graph and %d uniform pairs u != v' % (half, half)}


def child(a):
    """One library, one row: prints one JSON line."""
    import numpy as np
    from gem_amd.evaluation import link_heuristics as LH
    from gem_amd.graph import EdgeListGraph
    z = np.load(a.child)
    g = EdgeListGraph(int(z['n']), z['src'], z['dst'])
    st, ed = z['st'], z['ed']
    with LH.NeighbourScorer(g) as ns:
        first = ns.scores(st, ed)                                      # warm-up: code objects, the buffers' first allocation
        s0 = ns.stats()
        per = {k: [] for k in ('plan_ms', 'pair_upload_ms', 'kernel_ms', 'download_ms', 'scores_call_ms')}
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            got = ns.scores(st, ed)
            wall = (time.perf_counter() - t0) * 1e3
            s = ns.stats()
            for k in per:
                per[k].append(wall if k == 'scores_call_ms' else s[k])
        same = all(first[k].tobytes() == got[k].tobytes() for k in got)
    rec = {k: s0[k] for k in ('ingest_ms', 'graph_upload_ms', 'n', 'stored_neighbours', 'max_degree', 'lanes_per_narrow_group', 'narrow', 'chunk', 'narrow_items',
                              'wide_items', 'split_pairs', 'partial_slots', 'longest_item', 'pairs')}
    for k, v in per.items():
        rec[k] = float(np.median(v)); rec[k + '_min'] = float(min(v)); rec[k + '_max'] = float(max(v))
    rec.update({'warmup_kernel_ms': s0['kernel_ms'], 'repeats': a.repeats, 'calls_give_identical_bytes': bool(same), 'cn_sum': int(got['cn'].astype(np.int64).sum()),
                'aa_sum': float(got['aa'].sum()), 'pairs_per_s_kernel': len(st) / (rec['kernel_ms'] * 1e-3), 'pairs_per_s_scores_call': len(st) / (rec['scores_call_ms'] * 1e-3)})
    print('RESULT ' + json.dumps(rec), flush=True)


def run_child(lib, path, repeats):
    env = dict(os.environ)
    if lib:
        env['GEM_HIP_LIB'] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path, '--repeats', str(repeats)], env=env, stdout=subprocess.PIPE, universal_newlines=True,
                         timeout=600, check=True).stdout
    return json.loads([ln for ln in out.splitlines() if ln.startswith('RESULT ')][-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', default='sbm1m,rmat20,rmat22')
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--ab-libs', default='')
    ap.add_argument('--ab-rows', default='sbm1m,rmat20')
    ap.add_argument('--ab-rounds', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'link_baselines.json'))
    ap.add_argument('--child', default=None)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import numpy as np
    import nbr_refs as NB
    libs = [tuple(x.split('=', 1)) for x in a.ab_libs.split(',') if x]
    report = {'device': 'MI355X (gfx950)', 'host_threads': int(os.environ.get('OMP_NUM_THREADS', '0')), 'rows': {}, 'ab': {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name in [r for r in a.rows.split(',') if r]:
            t0 = time.perf_counter()
            g, st, ed, what = make_row(name)
            what['make_row_s'] = time.perf_counter() - t0
            path = os.path.join(tmp, name + '.npz')
            np.savez(path, n=g.n, src=g.src, dst=g.dst, st=st, ed=ed)
            rec = run_child(None, path, a.repeats)
            rec.update(what)
            pick = np.random.RandomState(1).permutation(len(st))[:SAMPLE]
            t0 = time.perf_counter()
            A = NB.simple_csr(g.n, g.src, g.dst)
            rec['scipy_csr_s'] = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref = NB.scores(A, st[pick], ed[pick])
            rec['scipy_scores_s'] = time.perf_counter() - t0
            rec['scipy_sample_pairs'] = int(len(pick))
            rec['scipy_pairs_per_s'] = len(pick) / rec['scipy_scores_s']
            rec['speedup_scores_call_vs_scipy'] = rec['pairs_per_s_scores_call'] / rec['scipy_pairs_per_s']
            report['rows'][name] = rec
            print(name, json.dumps(rec), flush=True)
            if libs and name in a.ab_rows.split(','):
                runs = {'tree': []}
                for _ in range(a.ab_rounds):                            # alternating: tree, variant 1, variant 2, ..., tree, ...
                    for label, lib in [('tree', None)] + libs:
                        r = run_child(lib, path, a.repeats)
                        assert r['cn_sum'] == rec['cn_sum'], (label, r['cn_sum'], rec['cn_sum'])
                        runs.setdefault(label, []).append({k: r[k] for k in ('lanes_per_narrow_group', 'narrow', 'chunk', 'narrow_items', 'wide_items', 'split_pairs',
                                                                              'kernel_ms', 'kernel_ms_min', 'kernel_ms_max', 'plan_ms', 'pair_upload_ms', 'scores_call_ms')})
                report['ab'][name] = runs
                print(name, 'ab', json.dumps(runs), flush=True)
            del g, st, ed, A, ref
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
