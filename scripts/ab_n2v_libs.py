"""node2vec on SBM-1024 on the library GEM_HIP_LIB selects: sha256 digests of everything deterministic -- walks and counts, the outputs of all four
unigram builders, single-wavefront SGNS tables at d = 16 / 128 / 130, one bucket of the two-partition schedule (two builds of the library must print
the same ones) -- and the median microseconds per gemhip_sgns_train call at d = 128 and the planner's width (CALLS Hogwild launches over the first
32 walks, each synchronised).  One JSON line.
    GEM_HIP_LIB=... python scripts/ab_n2v_libs.py
To compare two builds, each run a fresh child process under its own `timeout`, alternating, stopping at the first child that fails:
    python scripts/ab_n2v_libs.py --compare <parent libgem_hip.so> <branch libgem_hip.so> --out profiles/n2v_split_ab.json [--runs 7] [--bench 3]
--bench K also runs the default `python bench.py` line K times per library, alternating.  The branch's medians must lie inside the parent's min-max
spread or above it by less than that spread's width (exit status 1 otherwise, or when a digest differs)."""
import ctypes as C, hashlib, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import numpy as np

CALLS = int(os.environ.get('CALLS', 200))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def measure():
    from gem_amd import _hip
    from gem_amd.graph import to_csr
    L = _hip.lib()
    e = np.load(os.path.join(ROOT, 'tests', 'golden', 'sbm1024_edges.npy'))
    n, l, window, seed = 1024, 80, 10, 3
    row_ptr, col, _ = to_csr(n, e[:, 0].astype(np.int32), e[:, 1].astype(np.int32), None)
    h, m = C.c_void_p(), C.c_int64()
    i32, f32 = (lambda a: _hip.ptr(a, C.c_int32)), (lambda a: _hip.ptr(a, C.c_float))
    _hip.check(L.gemhip_n2v_create(n, len(col), _hip.ptr(row_ptr, C.c_int64), i32(col), None, C.byref(h)))
    _hip.check(L.gemhip_n2v_start_nodes(h, C.byref(m)))
    nwalks = m.value
    _hip.check(L.gemhip_n2v_walks(h, 1.0, 1.0, 1, l, seed, 11, 0, nwalks, None))
    walks = np.empty((nwalks, l), np.int32)
    _hip.check(L.gemhip_n2v_get_walks(h, i32(walks)))
    _hip.check(L.gemhip_n2v_vocab(h, None))
    out = {'lib': os.path.basename(os.path.dirname(os.path.abspath(_hip.LIB_PATH))) + '/' + os.path.basename(_hip.LIB_PATH), 'sha256': {}}
    D = out['sha256']
    # the four builders (the node-id single table last but one: the SGNS launches below draw from it)
    nv, order, UT, KT = C.c_int64(), np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32)
    _hip.check(L.gemhip_n2v_build_unigram_vocab_order(h, 11, C.byref(nv), i32(order), f32(UT), i32(KT)))
    D['build_unigram_vocab_order'] = sha(np.int64(nv.value), order, UT, KT)
    slot, nslots = np.zeros(n, np.int32), np.zeros(2, np.int64)
    _hip.check(L.gemhip_n2v_build_unigram_parts_vocab_order(h, 2, 11, None, 0, f32(UT), i32(KT), i32(slot), _hip.ptr(nslots, C.c_int64)))
    D['build_unigram_parts_vocab_order'] = sha(UT, KT, slot, nslots)
    counts = np.zeros(n, np.int32)
    _hip.check(L.gemhip_n2v_build_unigram(h, i32(counts), f32(UT), i32(KT)))
    D['walks'], D['counts'], D['build_unigram'] = sha(walks), sha(counts), sha(UT, KT)
    _hip.check(L.gemhip_n2v_build_unigram_parts(h, 2, f32(UT), i32(KT)))
    D['build_unigram_parts'] = sha(UT, KT)
    # deterministic launches on one wavefront
    for d in (16, 128, 130):
        P, N = np.empty((n, d), np.float32), np.empty((n, d), np.float32)
        _hip.check(L.gemhip_sgns_init(h, d, seed, None, None))
        _hip.check(L.gemhip_sgns_train(h, window, 5, 0.025, 1, 0, 0, nwalks, nwalks * l, 0, seed, 11 | 4, None))
        _hip.check(L.gemhip_sgns_get_tables(h, f32(P), f32(N)))
        D['sgns_det_d%d' % d] = sha(P, N)
    # one bucket (contexts of partition 0, centre words of partition 1) of the two-partition tables, d = 128, from the tables just trained
    d = 128
    Pp, Np = np.ascontiguousarray(P[0::2, :d]), np.ascontiguousarray(N[1::2, :d])
    dP, dN, dw = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for buf, host in ((dP, Pp), (dN, Np)):
        _hip.check(L.gemhip_malloc(C.byref(buf), host.nbytes))
        _hip.check(L.gemhip_memcpy_h2d(buf, host.ctypes.data_as(C.c_void_p), host.nbytes))
    _hip.check(L.gemhip_n2v_walks_ptr(h, C.byref(dw), None, None))
    _hip.check(L.gemhip_sgns_train_part(h, dw, nwalks, l, None, 0, 0, 0, window, 0.025, nwalks * l, 0, 0, seed, 11 | 4, 0, 1, dP, dN, d, None))
    _hip.check(L.gemhip_synchronize(None))
    for buf, host in ((dP, Pp), (dN, Np)):
        _hip.check(L.gemhip_memcpy_d2h(host.ctypes.data_as(C.c_void_p), buf, host.nbytes))
        _hip.check(L.gemhip_free(buf))
    D['sgns_part_bucket_0_1'] = sha(Pp, Np)
    # Hogwild calls at the planner's width, the plugin's table layout
    _hip.check(L.gemhip_n2v_build_unigram_vocab_order(h, 11, None, None, None, None))
    _hip.check(L.gemhip_sgns_init(h, 128, seed, None, None))
    us = []
    for rep in range(CALLS + 20):                            # the first 20 warm up
        _hip.check(L.gemhip_synchronize(None))
        t0 = time.perf_counter()
        _hip.check(L.gemhip_sgns_train(h, window, 5, 0.025, 1, 0, 0, 32, 32 * l, 0, seed + rep, 27, None))
        _hip.check(L.gemhip_synchronize(None))
        us.append((time.perf_counter() - t0) * 1e6)
    k, wv = C.c_int32(), C.c_int32()
    _hip.check(L.gemhip_sgns_last_launch(h, C.byref(k), C.byref(wv), None, None))
    _hip.check(L.gemhip_n2v_destroy(h))
    out.update(us_per_train_call=float(np.median(us[20:])), us_min=min(us[20:]), us_max=max(us[20:]), calls=CALLS, kernel=k.value, waves=wv.value)
    print(json.dumps(out), flush=True)


def child(lib, cmd, limit):
    """One fresh process on `lib` under its own time limit -> its last stdout line as JSON; raises when it fails."""
    run = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, env=dict(os.environ, GEM_HIP_LIB=lib), cwd=ROOT, stdout=subprocess.PIPE)
    if run.returncode != 0:
        raise SystemExit('%s on %s: exit status %d -- nothing further is started' % (' '.join(cmd), lib, run.returncode))
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


def verdict(parent, branch):
    lo, hi, med = min(parent), max(parent), float(np.median(branch))
    return {'parent': sorted(parent), 'branch': sorted(branch), 'parent_median': float(np.median(parent)), 'branch_median': med, 'parent_spread': hi - lo,
            'within': bool(lo <= med <= hi or hi < med < hi + (hi - lo))}


def compare(parent, branch, out_path, runs, bench):
    rec = {'what': 'scripts/ab_n2v_libs.py --compare on one MI355X: the parent commit\'s library and this one in alternating fresh processes; `within` = the '
                   'branch\'s median lies inside the parent\'s min-max spread or above it by less than the spread\'s width'}
    res = {'parent': [], 'branch': []}
    for i in range(runs):
        for name, lib in (('parent', parent), ('branch', branch)):
            res[name].append(child(lib, [sys.executable, os.path.abspath(__file__)], 300))
    digests = [r['sha256'] for r in res['parent'] + res['branch']]
    rec['sha256'] = digests[0]
    rec['digests_identical'] = all(dg == digests[0] for dg in digests)
    rec['launch'] = {'kernel': res['branch'][0]['kernel'], 'waves': res['branch'][0]['waves'], 'calls_per_process': res['branch'][0]['calls']}
    rec['us_per_train_call'] = verdict([r['us_per_train_call'] for r in res['parent']], [r['us_per_train_call'] for r in res['branch']])
    ok = rec['digests_identical'] and rec['us_per_train_call']['within']
    if bench:
        vals = {'parent': [], 'branch': []}
        for i in range(bench):
            for name, lib in (('parent', parent), ('branch', branch)):
                line = child(lib, [sys.executable, os.path.join(ROOT, 'bench.py')], 900)
                vals[name].append(line['value'])
                rec.setdefault('bench_metric', '%s [%s]' % (line['metric'], line['unit']))
        rec['bench_value'] = verdict(vals['parent'], vals['branch'])
        ok = ok and rec['bench_value']['within']
    with open(out_path, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps({k: v for k, v in rec.items() if k not in ('what', 'sha256')}, indent=1))
    return 0 if ok else 1


if __name__ == '__main__':
    if '--compare' in sys.argv:
        a = sys.argv
        at = a.index('--compare')
        opt = lambda name, default: int(a[a.index(name) + 1]) if name in a else default
        sys.exit(compare(os.path.abspath(a[at + 1]), os.path.abspath(a[at + 2]), a[a.index('--out') + 1], opt('--runs', 7), opt('--bench', 0)))
    measure()
