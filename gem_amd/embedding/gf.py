"""GraphFactorization on MI355X -- drop-in for gem.embedding.gf.GraphFactorization
(gem/embedding/gf.py:10-104).

learn_embedding() keeps the reference's contract (gf.py:81-101): falsy graph ->
ValueError('graph needed'); the embedding is initialised as 0.01*N(0,1) from
numpy's global RNG (so `np.random.seed` controls it exactly like the
reference); `max_iter` sequential sweeps over graph.edges() where only edges
with j > i fire and only row i is written; returns and stores the (n, d)
float64 array.  The sweeps run in libgem_hip.so (gem_amd/csrc/gf.hip) in fp32 --
the precision of the reference's own native path gem/c_src/gf.cpp.

Extra kwargs (backend knobs, kept on the instance): `seed`; `device_init` draws the
0.01*N(0,1) initial table on the GPU from a Philox stream keyed by `seed` (what
gf.cpp:41-52 does with its own generator) -- at 1M x 128 numpy's randn alone
costs more than 100 sweeps.  Default: ON when `seed` is given, OFF otherwise (a run
controlled by np.random.seed(), the reference's convention, keeps gf.py:92's numpy
draw); `device_init=False, seed=s` draws from a private RandomState(s).
`verbose=True` prints what the reference's native path prints (gf.cpp:144-151 run with
its verbose flag, as gf.py:62 does): before every `print_step`-th sweep the iteration
id and the objective f1 + f2 of gf.cpp:94-113 (f1 over all edges, f2 = ||X||_F^2),
also kept in `self._objective_log`.

`n_gpus=N` (with `devices=[...]` or `virtual_ranks=True`; gem_amd/embedding/_multi.py) shards the source rows over N GPUs -- one process driving N
devices through gemhip_gf_train_multi, or one process per GPU under torch.distributed -- with an all-gather of the owned row blocks after every sweep:
the same table as one GPU, bit for bit.

Edge order.  The default sweep kernel (one wavefront per source row) reproduces the reference's Gauss-Seidel order exactly with two
table copies, which needs every row a firing edge READS to have had all or none of its own updates of that sweep at that point of the
edge list.  That holds for graph.edges() of any networkx graph and for saveGraphToEdgeListTxt files (edges grouped by source) -- every
call site of the reference -- but not for arbitrary interleaved edge lists (a shuffled file, two sorted files concatenated, edges
appended later), which gf.cpp accepts.  By default libgem_hip.so then returns GEMHIP_E_INVALID (raised here as GemHipError) instead of
training something else.  Two opt-ins:
  * `exact_edge_order=True` trains graph.edges() / the EdgeListGraph arrays in exactly their order, whatever it is
    (gemhip_gf_plan_create_any_order): a list the row schedule represents gets the very same plan as without the kwarg; any other list
    gets the unit schedule (runs of one row's edges placed in dependency levels, DESIGN.md "GF: any edge order") -- the reference's
    result, at more launches per sweep.  `self._stats` records 'schedule' ('rows' or 'units'), 'levels' and 'units'.  A unit schedule
    is a single-device schedule: with n_gpus > 1 a list that needs it raises ValueError before any device call.
  * `regroup_edges=True` regroups the list by source (first-appearance order; gem_amd.graph.group_edges_by_source) -- fast, but a
    different visiting order than the reference's for that file.

`hub_block=True` runs the hub rows of a power-law graph (rows with at least GEMHIP_GF_HUB_EDGES firing edges, default 1024) B edges at a time through a
Gram matrix on the matrix units (gemhip_gf_plan_set_hub_block, DESIGN.md "GF: blocked hub rows"): the same updates within the fp32 tolerance of the
sequential loop, not bit-identical to the default schedule.  `self._stats` records 'hub_block' (the B in effect) and 'hub_rows'.  A single-GPU
kwarg: with n_gpus > 1 it raises ValueError before any device call (GEMHIP_GF_HUB_BLOCK=1 in the environment reaches the plans of every rank).
"""
import ctypes as C

import numpy as np

from gem_amd import _hip
from gem_amd.graph import edge_arrays
from gem_amd.embedding.static_graph_embedding import StaticGraphEmbedding


class GraphFactorization(StaticGraphEmbedding):
    hyper_params = {
        'print_step': 10000,
        'method_name': 'graph_factor_sgd',
    }

    def __init__(self, *args, **kwargs):
        super(GraphFactorization, self).__init__(*args, **kwargs)

    def learn_embedding(self, graph=None, edge_f=None, is_weighted=False, no_python=True, **_ignored):
        if not graph:
            raise ValueError('graph needed')
        import time
        t_begin = time.perf_counter()
        n, src, dst, w, _ = edge_arrays(graph)
        if getattr(self, '_regroup_edges', False):
            from gem_amd.graph import group_edges_by_source
            src, dst, w = group_edges_by_source(src, dst, w)
        exact = bool(getattr(self, '_exact_edge_order', False))
        if exact:
            from gem_amd.embedding import _multi
            from gem_amd.graph import row_schedule_represents
            if _multi.resolve(self)[0] != 'single' and not row_schedule_represents(src, dst):
                raise ValueError('exact_edge_order=True: this edge order needs the unit schedule, which is a single-device schedule; '
                                 'n_gpus=%r (train on one GPU, or regroup_edges=True if the reordering is acceptable)' % (getattr(self, '_n_gpus', 1),))
        hub_block = bool(getattr(self, '_hub_block', False))
        if hub_block:
            from gem_amd.embedding import _multi
            if _multi.resolve(self)[0] != 'single':
                raise ValueError('hub_block=True is a switch of the single-GPU plan; n_gpus=%r (set GEMHIP_GF_HUB_BLOCK=1 in the environment: every '
                                 'rank\'s plan reads it at creation)' % (getattr(self, '_n_gpus', 1),))
        t_ingested = time.perf_counter()
        d = int(self._d)
        self._node_num = n
        seed = getattr(self, '_seed', None)
        _hip.require_device()
        L = _hip.lib()
        verbose = bool(getattr(self, '_verbose', False))
        # n_gpus / devices / virtual_ranks kwargs (gem_amd/embedding/_multi.py): source rows sharded over N GPUs, all-gather of the owned blocks per sweep --
        # bit-identical to one GPU.  The initial table is gf.py:92's numpy draw (RandomState(seed), or numpy's global stream), identical on every rank
        from gem_amd.embedding import _multi
        mode, n_gpus, devices = _multi.resolve(self)
        if mode != 'single':
            if verbose:
                raise ValueError('verbose=True (the objective print of gf.cpp:144-151) is a single-GPU option; n_gpus=%d' % n_gpus)
            rng = np.random if seed is None else np.random.RandomState(seed)
            X0 = (0.01 * rng.randn(n, d)).astype(np.float32)          # gf.py:92
            if mode == 'spmd' and seed is None:                       # numpy's global stream differs between processes: rank 0's draw is everyone's
                X0 = _multi.broadcast_from_rank0(X0)
            t_init = time.perf_counter()
            self._stats = _multi.gf_capi(self, n, src, dst, w, X0, n_gpus, devices) if mode == 'capi' else _multi.gf_spmd(self, n, src, dst, w, X0)
            t_called = time.perf_counter()
            self._X = X0.astype(np.float64)
            self._api_wall = _hip.api_wall(t_begin, t_init, t_called, time.perf_counter())
            return self._X
        # device_init: explicit, else ON when `seed` is given (a seeded run does not need numpy's stream, and at 1M x 128 numpy's randn is 80 % of the
        # call: bench.py api_wall, round 4) -- np.random.seed()-controlled runs (no `seed` kwarg: the reference's own convention) keep gf.py:92's draw
        device_init = getattr(self, '_device_init', None)
        if device_init is None:
            device_init = seed is not None
        if device_init or verbose or exact or hub_block:
            X0 = np.empty((n, d), dtype=np.float32)
            plan = C.c_void_p()
            info = (C.c_int64 * 8)()
            wf = _hip.as_f32(w)
            if exact:
                _hip.check(L.gemhip_gf_plan_create_any_order(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32),
                                                             _hip.ptr(wf, C.c_float), d, 0, C.byref(plan)))
            else:
                _hip.check(L.gemhip_gf_plan_create(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32),
                                                   _hip.ptr(wf, C.c_float), d, 0, n, C.byref(plan)))
            t_plan = time.perf_counter()
            try:
                if hub_block:
                    _hip.check(L.gemhip_gf_plan_set_hub_block(plan, 1))
                if device_init:
                    _hip.check(L.gemhip_gf_plan_init_embedding(plan, int(seed if seed is not None else np.random.randint(2 ** 31 - 1)), 0.01))
                else:
                    rng = np.random if seed is None else np.random.RandomState(seed)
                    X0[:] = 0.01 * rng.randn(n, d)                    # gf.py:92
                    _hip.check(L.gemhip_gf_plan_set_embedding(plan, _hip.ptr(X0, C.c_float)))
                t_init = time.perf_counter()
                _hip.check(L.gemhip_gf_plan_info(plan, info))
                hub = (C.c_int32(0), C.c_int64(0))
                if hub_block:
                    _hip.check(L.gemhip_gf_plan_hub_block(plan, C.byref(hub[0]), C.byref(hub[1])))
                el, done, max_iter = 0.0, 0, int(self._max_iter)
                step = max(1, int(getattr(self, '_print_step', 10000))) if verbose else max(1, max_iter)
                self._objective_log = []
                while done < max_iter:
                    if verbose:
                        # gf.cpp:144-151: before every print_step-th sweep "\tIter id: k" and _print_f_value's line (gf.cpp:94-113: f1 over ALL edges, f2 = ||X||_F^2)
                        _hip.check(L.gemhip_gf_plan_get_embedding(plan, _hip.ptr(X0, C.c_float)))
                        f = (C.c_double * 2)()
                        _hip.check(L.gemhip_gf_objective(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(wf, C.c_float), d,
                                                         _hip.ptr(X0, C.c_float), f))
                        self._objective_log.append((done, f[0], f[1]))
                        print('\tIter id: %d' % done)
                        print('\t\tObjective: %g, f1: %g, f2:%g' % (f[0] + f[1], f[0], f[1]))
                    k = min(step, max_iter - done)
                    t0 = time.perf_counter()
                    _hip.check(L.gemhip_gf_plan_sweeps(plan, k, float(self._eta), float(self._regu), None))
                    _hip.check(L.gemhip_synchronize(None))
                    el += time.perf_counter() - t0
                    done += k
                t_d2h = time.perf_counter()
                _hip.check(L.gemhip_gf_plan_get_embedding(plan, _hip.ptr(X0, C.c_float)))
                t_got = time.perf_counter()
            finally:
                L.gemhip_gf_plan_destroy(plan)
            t_called = time.perf_counter()
            self._stats = {'kernel_seconds': el, 'updates_per_sweep': info[0], 'rows_per_sweep': info[1], 'levels': info[2]}
            if exact:
                self._stats.update({'schedule': 'units' if info[7] else 'rows', 'units': info[1]})
            if hub_block:
                self._stats.update({'hub_block': hub[0].value, 'hub_rows': hub[1].value})
            self._X = X0.astype(np.float64)
            t_end = time.perf_counter()
            # the breakdown of _hip.api_wall, stamped here: the staged calls are not one-shot drop-ins, gemhip_last_call_phases does not cover them
            self._api_wall = {'seconds': t_end - t_begin, 'ingest_s': t_ingested - t_begin, 'host_prepare_s': t_plan - t_ingested, 'h2d_s': t_init - t_plan,
                              'kernels_s': el, 'd2h_s': t_got - t_d2h, 'd2h_float64_s': (t_got - t_d2h) + (t_end - t_called), 'float64_copy_s': t_end - t_called,
                              'library_call_s': t_called - t_ingested, 'init': 'device (Philox)' if device_init else 'numpy randn + upload (counted as h2d_s)'}
            return self._X
        rng = np.random if seed is None else np.random.RandomState(seed)
        X0 = (0.01 * rng.randn(n, d)).astype(np.float32)          # gf.py:92
        t_init = time.perf_counter()
        stats = (C.c_double * 4)()
        _hip.check(L.gemhip_gf_train(n, len(src), _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32),
                                     _hip.ptr(_hip.as_f32(w), C.c_float), d, float(self._eta), float(self._regu),
                                     int(self._max_iter), _hip.ptr(X0, C.c_float), stats))
        t_called = time.perf_counter()
        self._stats = {'kernel_seconds': stats[0], 'updates_per_sweep': stats[1], 'rows_per_sweep': stats[2],
                       'levels': stats[3]}
        self._X = X0.astype(np.float64)
        # API wall: numpy's randn of gf.py:92 is part of learn_embedding on both sides; it is counted as ingest here
        self._api_wall = _hip.api_wall(t_begin, t_init, t_called, time.perf_counter())
        self._api_wall['numpy_randn_init_s'] = t_init - t_ingested
        return self._X

    def get_edge_weight(self, i, j):
        return np.dot(self._X[i, :], self._X[j, :])
