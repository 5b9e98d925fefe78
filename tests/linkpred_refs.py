"""Device-free inputs of the link-prediction GPU tests: a TRAIN mask for instrument_refs.ap_graph() (the 700-node TEST graph), and the host
order every device result is held against.  Operands, dense scores and the tie check are instrument_refs' own, unchanged.

The mask holds, by construction:
  node 2   (hub, 600 test neighbours, two chunks)   an EMPTY mask row
  node 5   (512 test neighbours)                    a mask row of 550 columns (longer than a chunk), 400 of them test neighbours
  node 9   (513 test neighbours)                    every column that is NOT a test neighbour: the candidates are exactly the positives, AP = 1
  LP_ALL_MASKED                                     every test neighbour masked: AP 0, no positive
  node 11  (empty test row)                         a mask row of three columns
  LP_UNSORTED                                       a mask row given as 500, 12, 500, 77 (unsorted, one column twice)
  LP_SELF                                           a masked self-loop (60 -> 60) next to 60 -> 61
  LP_LOWER                                          a mask row of lower ids only (never met when undirected)
and 3000 random arcs plus 500 of the test graph's own arcs on the remaining rows."""
import numpy as np

import instrument_refs as ir
from gem_amd.graph import to_csr

LP_ALL_MASKED, LP_UNSORTED, LP_SELF, LP_LOWER = 40, 30, 60, 300
LP_SPECIAL = (ir.AP_HUB, ir.AP_512, ir.AP_513, ir.AP_EMPTY, LP_ALL_MASKED, LP_UNSORTED, LP_SELF, LP_LOWER)


def lp_mask(truth):
    """(mask_row_ptr, mask_col, train_truth) for the test graph whose dense adjacency is `truth`; rows in the order given above (the CSR is
    NOT sorted: the library sorts and de-duplicates)."""
    n = ir.AP_N
    rng = np.random.RandomState(57)
    src = rng.randint(0, n, 3000); dst = rng.randint(0, n, 3000)
    ts, td = np.nonzero(truth)
    pick = rng.choice(len(ts), 500, replace=False)
    src = np.concatenate([src, ts[pick]]); dst = np.concatenate([dst, td[pick]])
    keep = ~np.isin(src, LP_SPECIAL)
    rows = [(src[keep], dst[keep])]

    def row(i, cols):
        rows.append((np.full(len(cols), i), np.asarray(cols)))
    nb5 = np.flatnonzero(truth[ir.AP_512]); other5 = np.setdiff1d(np.arange(n), nb5)
    row(ir.AP_512, rng.permutation(np.concatenate([rng.choice(nb5, 400, replace=False), rng.choice(other5, 150, replace=False)])))
    row(ir.AP_513, np.flatnonzero(~truth[ir.AP_513] & (np.arange(n) != ir.AP_513)))
    assert truth[LP_ALL_MASKED, LP_ALL_MASKED + 1:].sum() >= 1          # it has a neighbour that would rank when undirected
    row(LP_ALL_MASKED, np.flatnonzero(truth[LP_ALL_MASKED]))
    row(ir.AP_EMPTY, [3, 50, 600])
    row(LP_UNSORTED, [500, 12, 500, 77])
    row(LP_SELF, [LP_SELF, LP_SELF + 1])
    row(LP_LOWER, [1, 2, 3])
    src = np.concatenate([r[0] for r in rows]); dst = np.concatenate([r[1] for r in rows])
    row_ptr, col, _ = to_csr(n, src, dst, None)
    assert row_ptr[ir.AP_HUB + 1] == row_ptr[ir.AP_HUB] and row_ptr[ir.AP_512 + 1] - row_ptr[ir.AP_512] == 550
    assert list(col[row_ptr[LP_UNSORTED]:row_ptr[LP_UNSORTED + 1]]) == [500, 12, 500, 77]
    train = np.zeros((n, n), dtype=bool); train[src, dst] = True
    assert (train[ir.AP_512] & truth[ir.AP_512]).sum() == 400 and not (train[ir.AP_513] & truth[ir.AP_513]).any()
    return row_ptr, col, train


def candidate_order(score_row, i, undirected, train_row=None):
    """The candidates of node i in the evaluator's order: j != i, j > i when undirected, score > 0, not a train arc; score descending, id
    ascending on ties (the stable sort of the ascending-j list)."""
    n = score_row.shape[0]
    ok = score_row > 0
    ok[i] = False
    if undirected:
        ok[:i] = False
    if train_row is not None:
        ok &= ~train_row
    j = np.flatnonzero(ok)
    return j[np.argsort(-score_row[j], kind='stable')]


def npos_reference(score, train, truth, undirected):
    """Positives per node: test neighbours that are candidates."""
    n = score.shape[0]
    ok = (score > 0) & truth & ~train & ~np.eye(n, dtype=bool)
    if undirected:
        ok &= np.triu(np.ones((n, n), dtype=bool), 1)
    return ok.sum(axis=1)
