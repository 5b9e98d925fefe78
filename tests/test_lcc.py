"""CPU: gemhip_cc_labels / gemhip_lcc (gem_amd/csrc/cc.hip) refuse bad arguments on the host, before their first HIP call, and the Python
wrappers have no host fallback.  Validation only: nothing here needs a device."""
import ctypes as C

import numpy as np
import pytest

from gem_amd import _hip
from gem_amd.graph import EdgeListGraph


def i32(a):
    return None if a is None else np.array(a, np.int32)


def call_labels(n, src, dst, m=None, labels=True, ncomp=True):
    src, dst = i32(src), i32(dst)
    m = m if m is not None else len(src)
    out = np.full(min(max(n, 1), 16), -7, np.int32)              # (a refused call never looks at its size)
    nc = C.c_int32(-7)
    rc = _hip.lib().gemhip_cc_labels(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(out, C.c_int32) if labels else None,
                                     C.byref(nc) if ncomp else None)
    assert nc.value == -7 and np.all(out == -7), 'a refused call wrote to its outputs'
    return rc


def call_lcc(n, src, dst, m=None, w=None, drop=(), w_out=None):
    """drop: names of output pointers passed as NULL."""
    src, dst = i32(src), i32(dst)
    m = m if m is not None else len(src)
    size = min(max(n, 1), 16)                                        # (a refused call never looks at the sizes)
    bufs = {'old_of_new': np.full(size, -7, np.int32), 'new_of_old': np.full(size, -7, np.int32), 'src_out': np.full(min(max(m, 1), 16), -7, np.int32),
            'dst_out': np.full(min(max(m, 1), 16), -7, np.int32)}
    n_out, m_out, nc = C.c_int64(-7), C.c_int64(-7), C.c_int32(-7)
    p = {k: (None if k in drop else _hip.ptr(v, C.c_int32)) for k, v in bufs.items()}
    rc = _hip.lib().gemhip_lcc(n, m, _hip.ptr(src, C.c_int32), _hip.ptr(dst, C.c_int32), _hip.ptr(w, C.c_float),
                               None if 'n_out' in drop else C.byref(n_out), None if 'm_out' in drop else C.byref(m_out), p['old_of_new'], p['new_of_old'],
                               p['src_out'], p['dst_out'], _hip.ptr(w_out, C.c_float), None if 'n_components' in drop else C.byref(nc))
    assert (n_out.value, m_out.value, nc.value) == (-7, -7, -7) and all(np.all(v == -7) for v in bufs.values()), 'a refused call wrote to its outputs'
    return rc


BAD_ARCS = (([0, 1, 2, 9], [1, 5, 2, 0], b'%s: edge 1 = (1,5) outside [0,5)'),          # dst == n; a later arc is worse: the FIRST offender is named
            ([0, 4, 5], [1, 4, 0], b'%s: edge 2 = (5,0) outside [0,5)'),                # src == n (the self-loop (4,4) is fine)
            ([0, -1], [1, 2], b'%s: edge 1 = (-1,2) outside [0,5)'),
            ([0, 1], [1, -2147483648], b'%s: edge 1 = (1,-2147483648) outside [0,5)'))


def test_cc_labels_refuses_bad_arguments_before_any_device_call():
    L = _hip.lib()
    for src, dst, msg in BAD_ARCS:
        assert call_labels(5, src, dst) == _hip.E_INVALID
        assert L.gemhip_last_error() == msg % b'cc_labels'
    for src, dst in ((None, [1, 2]), ([1, 2], None), (None, None)):
        assert call_labels(5, src, dst, m=2) == _hip.E_INVALID
        assert L.gemhip_last_error() == b'cc_labels: bad edge arrays'
    assert call_labels(5, [0], [1], labels=False) == _hip.E_INVALID
    assert L.gemhip_last_error() == b'cc_labels: NULL output'
    assert call_labels(5, [0], [1], ncomp=False) == _hip.E_INVALID
    assert call_labels(0, [], [], m=0) == _hip.E_INVALID
    assert L.gemhip_last_error() == b'cc_labels: n = 0, m = 0 (need n >= 1, m >= 0)'
    assert call_labels(5, [0], [1], m=-1) == _hip.E_INVALID
    assert call_labels(1 << 31, [0], [1]) == _hip.E_UNSUPPORTED
    assert call_labels(5, [0], [1], m=1 << 31) == _hip.E_UNSUPPORTED
    assert L.gemhip_last_error() == b'cc_labels: n = 5, m = 2147483648: both must be below 2^31'


def test_lcc_refuses_bad_arguments_before_any_device_call():
    L = _hip.lib()
    for src, dst, msg in BAD_ARCS:
        assert call_lcc(5, src, dst) == _hip.E_INVALID
        assert L.gemhip_last_error() == msg % b'lcc'
    for src, dst in ((None, [1, 2]), ([1, 2], None), (None, None)):
        assert call_lcc(5, src, dst, m=2) == _hip.E_INVALID
        assert L.gemhip_last_error() == b'lcc: bad edge arrays'
    for name in ('n_out', 'm_out', 'old_of_new', 'new_of_old', 'src_out', 'dst_out', 'n_components'):
        assert call_lcc(5, [0], [1], drop=(name,)) == _hip.E_INVALID
        assert L.gemhip_last_error() == b'lcc: NULL output'
    one = np.ones(1, np.float32)
    assert call_lcc(5, [0], [1], w=one) == _hip.E_INVALID                 # weights in, nowhere to put them
    assert L.gemhip_last_error() == b'lcc: w and w_out go together (both given or both NULL)'
    assert call_lcc(5, [0], [1], w_out=one) == _hip.E_INVALID and one[0] == 1.0
    assert call_lcc(0, [], [], m=0) == _hip.E_INVALID
    assert L.gemhip_last_error() == b'lcc: n = 0, m = 0 (need n >= 1, m >= 0)'
    assert call_lcc(1 << 31, [0], [1]) == _hip.E_UNSUPPORTED
    assert call_lcc(5, [0], [1], m=1 << 31) == _hip.E_UNSUPPORTED


def test_python_wrappers_have_no_host_fallback():
    """Without a device connected_components, largest_component, get_lcc and evaluateStaticLinkPrediction(lcc=True) raise, like every product path."""
    from gem_amd import graph
    from gem_amd.embedding.gf import GraphFactorization
    from gem_amd.evaluation.link_prediction import evaluateStaticLinkPrediction
    from gem.utils import graph_util
    if _hip.device_count() > 0:
        pytest.skip('GPU present')
    g = EdgeListGraph(4, [0, 1], [1, 2])
    for fn in (graph.connected_components, graph.largest_component, graph_util.get_lcc):
        with pytest.raises(_hip.GemHipError):
            fn(g)
    with pytest.raises(_hip.GemHipError):
        graph_util.get_lcc(g.to_networkx())
    with pytest.raises(_hip.GemHipError):
        evaluateStaticLinkPrediction(g, GraphFactorization(d=2, eta=0.1, regu=0.1, max_iter=1), train_ratio=0.5, lcc=True)
