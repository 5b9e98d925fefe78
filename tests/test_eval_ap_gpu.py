"""GPU: gemhip_eval_ap at EVERY eval_ap_kernel<NV, KIND, false> instantiation (NV = 1, 2, 4, 8; inner product and distance kernel), node by node against
gr.average_precision_rows on the dense fp64 score matrix of the same fp32 inputs, with and without `undirected`, over all 700 nodes of
instrument_refs.ap_graph (a hub of 600 = two chunks, rows of 512 and 513, an empty row, a row of lower ids only, an unsorted row that lists a
column twice).  Widths on either side of every NV boundary and tail mask, ld > da with 1e30 in the padding, HOPE splits wider than 16.
Two input families: half-integer grid values (every score exact, exact ties everywhere: 1e-12) and random fp32 values (the project's 1e-9,
after checking on the CPU that the fp64 reference itself is clear of ties).  test_instrument_refs.py shows on the CPU that a lost column or a
lost neighbour moves these APs by more than 1e-4."""
import ctypes as C

import numpy as np
import pytest

import instrument_refs as ir
from gem_amd import _hip
from gem_amd.evaluation import reconstruction as gr
from test_eval_pairs_gpu import Handle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ap_graph():
    return ir.ap_graph()


@pytest.mark.parametrize('family', ['grid', 'random'])
@pytest.mark.parametrize('da,pad,kind,split', ir.AP_CASES)
def test_ap_of_every_node_at_every_instantiation(ap_graph, da, pad, kind, split, family):
    row_ptr, col, truth = ap_graph
    n = ir.AP_N
    bar = ir.AP_GRID_BAR if family == 'grid' else ir.AP_RANDOM_BAR
    A, B = ir.ap_operands(da, pad, kind, split, family, seed=ir.ap_seed(da, kind))
    score, mag = ir.ap_dense_scores(A, B, da, kind)
    if family == 'random':
        assert ir.ap_reference_is_clear_of_ties(score, mag, da), 'the fp64 reference does not decide an order at this seed: pick another'
    nodes = np.arange(n, dtype=np.int32)
    with Handle(n, da, da + pad, A, B, kind, row_ptr, col) as h:
        got = {und: h.ap(nodes, und) for und in (True, False)}
        again = h.ap(nodes, False)
    assert again.tobytes() == got[False].tobytes()                                # two calls on one handle: the same bytes
    for und in (True, False):
        ref = gr.average_precision_rows(score, truth, undirected=und)
        err = np.abs(got[und] - ref)
        print('AP %s kind %d da=%d ld=%d split=%d undirected=%d: max |AP - ref| = %.3g at node %d (bar %.0e), MAP %.6f'
              % (family, kind, da, da + pad, split, und, err.max(), int(err.argmax()), bar, got[und].mean()))
        assert np.all(err <= bar)
        assert ref[ir.AP_EMPTY] == 0.0 and got[und][ir.AP_EMPTY] == 0.0 and (not und or got[und][ir.AP_LOWER] == 0.0)
        assert da == 1 or ref[[ir.AP_HUB, ir.AP_512, ir.AP_513]].min() > 0.0        # the chunked rows are really scored
        if kind == 1 and family == 'grid':                                          # the row moved away: exp underflows, it ranks nothing and nobody ranks it
            assert np.all(score[ir.AP_FAR] == 0.0) and np.all(score[:, ir.AP_FAR] == 0.0) and got[und][ir.AP_FAR] == 0.0


def test_ap_small_cases(ap_graph):
    row_ptr, col, truth = ap_graph
    A, _ = ir.ap_operands(65, 0, 0, False, 'random', seed=1)
    L = _hip.lib()
    with Handle(ir.AP_N, 65, 65, A, None, 0, row_ptr, col) as h:
        _hip.check(L.gemhip_eval_ap(h.h, 1, 0, None, None))                          # nsample = 0 is legal
        twice = h.ap(np.array([ir.AP_HUB, 40, ir.AP_HUB, 40], np.int32), True)
        once = h.ap(np.array([ir.AP_HUB, 40], np.int32), True)
    assert twice[0] == twice[2] and twice[1] == twice[3] and twice[:2].tobytes() == once.tobytes() and once[0] > 0
    # node 0's true neighbours 1 and 2 score -1 and 0, the strangers 3 and 4 score 2 and 1: nothing of node 0's is ranked -> AP 0
    X = np.array([[1.0], [-1.0], [0.0], [2.0], [1.0]], np.float32)
    rp = np.array([0, 2, 3, 3, 3, 3], np.int64); cl = np.array([1, 2, 3], np.int32)
    t5 = np.zeros((5, 5), dtype=bool); t5[0, 1] = t5[0, 2] = t5[1, 3] = True
    with Handle(5, 1, 1, X, None, 0, rp, cl) as h:
        for und in (True, False):
            ap = h.ap(np.arange(5, dtype=np.int32), und)
            ref = gr.average_precision_rows(X.astype(np.float64) @ X.astype(np.float64).T, t5, undirected=und)
            assert ap[0] == 0.0 and np.array_equal(ap, ref)
