"""Three-way timing of GF's blocked hub rows (gemhip_gf_plan_set_hub_block, DESIGN.md "GF: blocked hub rows") -> profiles/gf_hub_block.json.

    timeout -k 10 <limit> python scripts/ab_gf_hub_block.py --parent-lib <libgem_hip.so of the parent commit> [--graphs rmat22,rmat20,sbm1m] [--out FILE]

Per graph (R-MAT scale 22 and 20 at 16 edges per node, SBM 1M/10M; d = 128, eta = 1e-4, regu = 1) three arms, each in a process of its own that loads
its library with ctypes and binds only the calls it uses -- so the parent's library is driven through calls the parent exports:
  (a) the parent commit's library, (b) this build with the switch off, (c) this build with the switch on.
Every arm draws the same initial table on the device (Philox, seed 1), runs 5 sweeps to warm up, draws the table again and times 3 repeats of 100
sweeps with device events on the stream the sweeps run on (the first repeat ends exactly 100 sweeps after the start: its table is kept).  Recorded:
ms per sweep of every repeat, the spread of (a)'s repeats, whether (b) agrees with (a) within that spread, (a)/(c), the largest deviation between
the tables of (b) and (c) after 100 sweeps (relative to max|X|; on SBM, which has no hub rows, the tables must be equal), and with --oracle-sweeps N
(default 4, R-MAT-22 only) both modes against the sequential fp32 CPU loop after N sweeps.  The graph is generated once and handed to the arms in a file."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

D, ETA, REGU, SWEEPS, REPEATS, SEED = 128, 1e-4, 1.0, 100, 3, 1


def make_graph(name):
    from gem_amd.graph import edge_arrays, rmat_graph, sbm_graph
    if name.startswith('rmat'):
        scale = int(name[4:])
        g = rmat_graph(scale, 16 << scale, seed=20260923 + 5)
    elif name == 'sbm1m':
        g = sbm_graph(1000000, 10000000, 100, seed=20260923 + 4)
    else:
        raise SystemExit('unknown graph %r' % name)
    n, src, dst, _, _ = edge_arrays(g)
    return n, np.ascontiguousarray(src, np.int32), np.ascontiguousarray(dst, np.int32)


def load_lib(path):
    L = C.CDLL(path)
    i32p, f32p, vp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p
    sigs = {'gemhip_gf_plan_create': [C.c_int64, C.c_int64, i32p, i32p, f32p, C.c_int32, C.c_int64, C.c_int64, C.POINTER(vp)],
            'gemhip_gf_plan_destroy': [vp], 'gemhip_gf_plan_init_embedding': [vp, C.c_uint64, C.c_float],
            'gemhip_gf_plan_sweeps': [vp, C.c_int32, C.c_float, C.c_float, vp], 'gemhip_gf_plan_get_embedding': [vp, f32p],
            'gemhip_gf_plan_info': [vp, C.POINTER(C.c_int64)], 'gemhip_synchronize': [vp]}
    if hasattr(L, 'gemhip_gf_plan_set_hub_block'):
        sigs.update({'gemhip_gf_plan_set_hub_block': [vp, C.c_int32], 'gemhip_gf_plan_hub_block': [vp, i32p, C.POINTER(C.c_int64)]})
    for name, args in sigs.items():
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = args
    L.gemhip_last_error.restype = C.c_char_p
    return L


def child(args):
    """one library, the modes asked for in turn; one JSON line"""
    import torch
    L = load_lib(args.lib)

    def ok(rc):
        if rc:
            raise SystemExit('library error %d: %s' % (rc, L.gemhip_last_error().decode()))
    z = np.load(args.child)
    n, src, dst = int(z['n']), z['src'], z['dst']
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = {'lib': args.lib, 'modes': {}}
    tables = {}
    for mode in args.modes.split(','):
        plan = C.c_void_p()
        ok(L.gemhip_gf_plan_create(n, len(src), p32(src), p32(dst), None, D, 0, n, C.byref(plan)))
        rec = {}
        if mode == 'on':
            ok(L.gemhip_gf_plan_set_hub_block(plan, 1))
        if hasattr(L, 'gemhip_gf_plan_hub_block'):
            b = C.c_int32(); hubs = C.c_int64()
            ok(L.gemhip_gf_plan_hub_block(plan, C.byref(b), C.byref(hubs)))
            rec.update(block=b.value, hub_rows=hubs.value)
        info = (C.c_int64 * 8)()
        ok(L.gemhip_gf_plan_info(plan, info))
        rec.update(updates_per_sweep=info[0], rows=info[1], levels=info[2])
        X = np.empty((n, D), np.float32)
        xp = X.ctypes.data_as(C.POINTER(C.c_float))
        if args.oracle_sweeps > 0:
            ok(L.gemhip_gf_plan_init_embedding(plan, SEED, 0.01))
            if 'X0' not in tables:
                ok(L.gemhip_gf_plan_get_embedding(plan, xp))
                tables['X0'] = X.copy()
            ok(L.gemhip_gf_plan_sweeps(plan, args.oracle_sweeps, ETA, REGU, None))
            ok(L.gemhip_gf_plan_get_embedding(plan, xp))
            tables['oracle_' + mode] = X.copy()
        ok(L.gemhip_gf_plan_init_embedding(plan, SEED, 0.01))
        ok(L.gemhip_gf_plan_sweeps(plan, 5, ETA, REGU, None))                     # warm-up
        ok(L.gemhip_gf_plan_init_embedding(plan, SEED, 0.01))
        ok(L.gemhip_synchronize(None))
        ms = []
        for rep in range(REPEATS):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()                                                          # torch's current stream is the null stream, the one the sweeps run on
            ok(L.gemhip_gf_plan_sweeps(plan, SWEEPS, ETA, REGU, None))
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1) / SWEEPS)
            if rep == 0:
                ok(L.gemhip_gf_plan_get_embedding(plan, xp))
                rec['sha256_after_100'] = hashlib.sha256(X.tobytes()).hexdigest()
                rec['finite'] = bool(np.isfinite(X).all())
                tables[mode] = X.copy()
        rec['ms_per_sweep'] = ms
        ok(L.gemhip_gf_plan_destroy(plan))
        out['modes'][mode] = rec
    if 'off' in tables and 'on' in tables:
        scale = float(np.abs(tables['off']).max())
        out['on_vs_off_after_100'] = {'max_abs': float(np.abs(tables['on'] - tables['off']).max()), 'scale_max_abs_X': scale}
        out['on_vs_off_after_100']['relative'] = out['on_vs_off_after_100']['max_abs'] / scale
    if args.oracle_sweeps > 0:
        import oracle
        t = time.time()
        ref = oracle.gf_train_f32(n, src, dst, None, D, ETA, REGU, args.oracle_sweeps, tables['X0'])
        scale = float(np.abs(ref).max())
        out['vs_cpu_fp32_loop'] = {'sweeps': args.oracle_sweeps, 'scale_max_abs_ref': scale, 'cpu_seconds': time.time() - t}
        for mode in args.modes.split(','):
            out['vs_cpu_fp32_loop'][mode + '_relative'] = float(np.abs(tables['oracle_' + mode] - ref).max()) / scale
    print(json.dumps(out), flush=True)


def run_child(lib, graph_file, modes, oracle_sweeps, limit):
    cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--child', graph_file, '--lib', lib, '--modes', modes,
           '--oracle-sweeps', str(oracle_sweeps)]
    run = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE)
    if run.returncode != 0:
        raise SystemExit('arm %s of %s ended with status %d: nothing more is started' % (modes, lib, run.returncode))
    return json.loads(run.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib'); ap.add_argument('--graphs', default='rmat22,rmat20,sbm1m')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gf_hub_block.json'))
    ap.add_argument('--oracle-sweeps', type=int, default=4); ap.add_argument('--limit', type=int, default=500)
    ap.add_argument('--child'); ap.add_argument('--lib'); ap.add_argument('--modes', default='off')
    args = ap.parse_args()
    if args.child:
        return child(args)
    from gem_amd import _hip
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    result.update({'d': D, 'eta': ETA, 'regu': REGU, 'sweeps_per_repeat': SWEEPS, 'repeats': REPEATS})
    result.setdefault('graphs', {})
    with tempfile.TemporaryDirectory() as tmp:
        for name in args.graphs.split(','):
            t = time.time()
            n, src, dst = make_graph(name)
            gfile = os.path.join(tmp, name + '.npz')
            np.savez(gfile, n=n, src=src, dst=dst)
            print('%s: n=%d m=%d generated in %.0f s' % (name, n, len(src), time.time() - t), flush=True)
            a = run_child(os.path.abspath(args.parent_lib), gfile, 'off', 0, args.limit)
            bc = run_child(_hip.LIB_PATH, gfile, 'off,on', args.oracle_sweeps if name == 'rmat22' else 0, args.limit)
            os.remove(gfile)
            ta, tb, tc = a['modes']['off']['ms_per_sweep'], bc['modes']['off']['ms_per_sweep'], bc['modes']['on']['ms_per_sweep']
            med = lambda v: float(np.median(v))
            spread = max(ta) - min(ta)
            g = {'n': n, 'edges': int(len(src)), 'a_parent': a['modes']['off'], 'b_off': bc['modes']['off'], 'c_on': bc['modes']['on'],
                 'a_spread_ms': spread, 'b_within_a_spread': bool(min(ta) - spread <= med(tb) <= max(ta) + spread),
                 'b_table_equals_a': a['modes']['off']['sha256_after_100'] == bc['modes']['off']['sha256_after_100'],
                 'c_table_equals_b': bc['modes']['on']['sha256_after_100'] == bc['modes']['off']['sha256_after_100'],
                 'median_ms': {'a': med(ta), 'b': med(tb), 'c': med(tc)}, 'a_over_c': med(ta) / med(tc),
                 'c_below_a_by_more_than_spread': bool(med(tc) < med(ta) - spread), 'on_vs_off_after_100': bc['on_vs_off_after_100']}
            if 'vs_cpu_fp32_loop' in bc:
                g['vs_cpu_fp32_loop'] = bc['vs_cpu_fp32_loop']
            result['graphs'][name] = g
            print(json.dumps({name: {k: g[k] for k in ('median_ms', 'a_spread_ms', 'a_over_c', 'b_within_a_spread', 'c_table_equals_b')}}), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, 'w') as f:
                json.dump(result, f, indent=1, sort_keys=True)
                f.write('\n')


if __name__ == '__main__':
    main()
