"""gemhip_lap_eigmap and gemhip_lle on weighted graphs with self-loops, zero-degree nodes inside the node order, several components, negative
weights (LLE) and the 6-node edge-case graph, on both solvers, against fp64 dense references (lap_lle_refs.py; bars and measured values:
tests/README_lap_lle.md).  All k columns are checked, the trivial ones included -- the classes drop column 0."""
import ctypes as C

import numpy as np
import pytest

import lap_lle_refs as refs
from conftest import golden_path
from gem_amd import _hip
from gem_amd.embedding.lap import LaplacianEigenmaps, symmetric_arrays
from gem_amd.embedding.lle import LocallyLinearEmbedding
from gem_amd.graph import to_csr

pytestmark = pytest.mark.gpu

OVERSAMPLE = 16
KINDS = {'weighted': ('lap', 'lle'), 'isolated': ('lap', 'lle'), 'components': ('lap', 'lle'), 'tiny': ('lap', 'lle'), 'signed': ('lle',)}


def device(kind, graph, k):
    """The entry point called as lap.py / lle.py call it: (V [n][k], operator eigenvalues (lle: s^2), the values as returned, solver, stats)."""
    n, src, dst, w = symmetric_arrays(graph)
    row_ptr, col, ww = to_csr(n, src, dst, w)
    V = np.empty((n, k), np.float32); vals = np.empty(k, np.float32)
    stats = (C.c_double * 12)()
    fn, restarts = (_hip.lib().gemhip_lap_eigmap, 30) if kind == 'lap' else (_hip.lib().gemhip_lle, 40)
    _hip.check(fn(n, len(col), _hip.ptr(row_ptr, C.c_int64), _hip.ptr(col, C.c_int32), _hip.ptr(ww, C.c_float), k, OVERSAMPLE, 3, restarts, 1e-6, 20260923,
                  _hip.ptr(V, C.c_float), _hip.ptr(vals, C.c_float), stats))
    lam = vals.astype(np.float64) if kind == 'lap' else vals.astype(np.float64) ** 2
    return V, lam, vals, 'eigen-path' if stats[3] < 0 else 'block-Krylov', list(stats)


def cases():
    for name in sorted(KINDS):
        for kind in KINDS[name]:
            for d in refs.CASE_D[name]:
                for sym in ('0', '1'):
                    if sym == '0' or d + 1 + OVERSAMPLE + 1 < len(refs.case_graph(name)):          # solve_operator's condition for the eigen-path
                        yield kind, name, d, sym


@pytest.mark.parametrize('kind,name,d,sym', list(cases()))
def test_against_the_fp64_reference(kind, name, d, sym, monkeypatch):
    monkeypatch.setenv('GEMHIP_HOPE_SYM', sym)
    V, lam, vals, solver, stats = device(kind, refs.case_graph(name), d + 1)
    label = '%s %s d=%d GEMHIP_HOPE_SYM=%s answered by %s (%d cycles)' % (kind, name, d, sym, solver, stats[5])
    if sym == '0' or name == 'weighted':
        assert solver == ('eigen-path' if sym == '1' else 'block-Krylov'), label         # (degenerate graphs may fall back by design: recorded above)
    refs.check(label, refs.reference(kind, name), V, lam, refs.CASE_CUTS[name])
    assert np.all(np.diff(vals) >= 0), vals


@pytest.mark.parametrize('kind', ['lap', 'lle'])
def test_classes_return_the_direct_call_without_column_0(kind, monkeypatch):
    monkeypatch.delenv('GEMHIP_HOPE_SYM', raising=False)
    G, small, d = refs.isolated(), refs.tiny(), 3
    m = (LaplacianEigenmaps if kind == 'lap' else LocallyLinearEmbedding)(d=d)
    Y = m.learn_embedding(graph=G)
    V, lam, vals, solver, _ = device(kind, G, d + 1)
    assert Y.shape == (len(G), d) and Y.dtype == np.float64 and np.array_equal(Y, V[:, 1:].astype(np.float64))
    got = m._eigvals if kind == 'lap' else m._singvals
    assert got.shape == (d + 1,) and np.array_equal(got, vals.astype(np.float64)) and np.all(np.diff(got) > 0)
    assert m._stats['solver'] == 'block_krylov' and solver == 'block-Krylov'

    def no_device(*a, **kw):
        raise AssertionError('d = n - 1 must be refused before the device is touched')
    monkeypatch.setattr(_hip, 'lib', no_device); monkeypatch.setattr(_hip, 'require_device', no_device)
    for g in (G, small):
        with pytest.raises(ValueError):
            (LaplacianEigenmaps if kind == 'lap' else LocallyLinearEmbedding)(d=len(g) - 1).learn_embedding(graph=g)


@pytest.mark.parametrize('which', ['asym', 'tiny'])
@pytest.mark.parametrize('kind', ['lap', 'lle'])
def test_edge_list_and_digraph_are_one_graph(kind, which, monkeypatch):
    """The EdgeListGraph and its to_networkx() DiGraph: both against the fp64 reference of networkx's symmetrisation, and against each other
    within the same bars (not bytes: the column order within CSR rows may differ)."""
    monkeypatch.setenv('GEMHIP_HOPE_SYM', '0')
    g = refs.asym() if which == 'asym' else refs.tiny()
    d, cuts = (3, (1, 4)) if which == 'asym' else (4, refs.CASE_CUTS['tiny'])
    ref = refs.reference_of(kind, refs.adjacency(g))
    out = []
    for label, graph in (('EdgeListGraph', g), ('DiGraph', g.to_networkx())):
        V, lam, _, solver, _ = device(kind, graph, d + 1)
        refs.check('%s %s d=%d %s' % (kind, which, d, label), ref, V, lam, cuts)
        out.append((V.astype(np.float64), lam))
    (Va, la), (Vb, lb) = out
    dv, bar = float(np.abs(la - lb).max()), ref.value_bar(d + 1)[0]
    print('%s %s: containers: values differ by %.3e [bar %.3e]' % (kind, which, dv, bar))
    assert dv <= bar
    for j in cuts:
        ang, bar = float(np.linalg.norm(Vb[:, :j] - Va[:, :j] @ (Va[:, :j].T @ Vb[:, :j]), 2)), ref.subspace_bar(j)[0]
        print('%s %s: containers: subspaces at cut %d differ by %.3e [bar %.3e]' % (kind, which, j, ang, bar))
        assert ang <= bar


@pytest.mark.parametrize('name,d', [('weighted', 3), ('isolated', 3), ('tiny', 1), ('tiny', 2)])
def test_device_spans_what_the_reference_returned(name, d, monkeypatch):
    """[V[:, 0] | Y] of the device against the reference implementation's own LaplacianEigenmaps output (tests/golden/ref_lap_edges.npz)."""
    monkeypatch.setenv('GEMHIP_HOPE_SYM', '0')
    gold = np.load(golden_path('ref_lap_edges.npz'))['%s_d%d' % (name, d)]
    V = device('lap', refs.case_graph(name), d + 1)[0].astype(np.float64)
    gold = gold / np.linalg.norm(gold, axis=0)
    dist, bar = float(np.linalg.norm(gold - V @ (V.T @ gold), axis=0).max()), refs.reference('lap', name).subspace_bar(d + 1)[0]
    print('lap %s d=%d: reference output from the device span %.3e [bar %.3e]' % (name, d, dist, bar))
    assert dist <= bar
