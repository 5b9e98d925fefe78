"""Writes the node-classification fixtures under tests/golden/ (tests/README_nc.md).  CPU only; needs scikit-learn (1.7.2 when the fixtures
were made).

    python scripts/make_golden_nc.py

nc_ref.npz    per data set of tests/nc_refs.py data_sets(): W_<name> [K][d + 1] fp64, w then b -- sklearn
              LogisticRegression(solver='newton-cholesky', tol=1e-12, max_iter=1000) per class on the set's training rows.
nc_ref.json   per prediction set the micro-F1, macro-F1 and accuracy of the top-k ranker on the exact minimiser and on
              OneVsRestClassifier(LogisticRegression(max_iter=1000)); per set the figures the asserted conditions were checked with.

Inputs are NOT stored: nc_refs rebuilds them from hope_sbm1024_d32.npz, sbm1024_labels.npy and seeds.  Asserted here, because the tests
rest on it: (a) on the sets whose coefficients a test compares (COEFFICIENT_SETS) the fp64 restatement, run to dec_tol = 1e-12, equals
sklearn's newton-cholesky to 1e-12 of max |theta*|; (b) on each prediction set the smallest
k-th / (k+1)-th probability gap is at least 4 x the float32 restatement's largest probability deviation; (c) on the line-search sets the
fp64 restatement backtracks at least once; (d) on the prediction sets the default-settings classifier predicts what the exact minimiser does.

On (a).  sklearn scales its objective by 1 / (C n), so its tol = 1e-12 is about 1e-9 on the gradient of F and it can stop one Newton step
before the fp64 floor; the restatement at the solver's default dec_tol = 1e-10 can too.  Against a minimiser polished in extended precision
the restatement at dec_tol = 1e-12 is within 1e-14 on every set, sklearn within 3e-12.  `x100` is a prediction set only: sklearn's stop
leaves it 2e-12 from the restatement (recorded, not asserted).  The seeds of nc_refs: the label draw of `normal` (20) is the first of
18.. on which the C = 1e4 fit backtracks and (a) holds at both C; the draw of `warm` (26) is the one of 17..26 closest in (a); the
synthetic classes (5) and the split (0) were never changed."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REFERENCE_DEC_TOL = 1e-12
COEFFICIENT_SETS = ('std', 'raw', 'normal', 'normal_C1e4', 'warm')


def main():
    import sklearn
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier
    from sklearn.metrics import accuracy_score, f1_score
    import nc_refs as R

    arrays, report = {}, {'sklearn': sklearn.__version__, 'sets': {}}
    for name, ds in R.data_sets().items():
        X, Y, C = ds['X'], ds['Y'], ds['C']
        n, K = Y.shape
        train = R.train_rows(name, n)
        Xt, Yt = X[train].astype(np.float64), Y[train]
        W = np.zeros((K, X.shape[1] + 1))
        for c in range(K):
            m = LogisticRegression(C=C, solver='newton-cholesky', tol=1e-12, max_iter=1000).fit(Xt, Yt[:, c])
            W[c, :-1], W[c, -1] = m.coef_[0], m.intercept_[0]
        W64, info64 = R.fit_all(X[train], Yt, C, ds['W0'], np.float64, dec_tol=REFERENCE_DEC_TOL)
        W64d = R.fit_all(X[train], Yt, C, ds['W0'], np.float64)[0]                            # the solver's default dec_tol = 1e-10
        W32, info32 = R.fit_all(X[train], Yt, C, ds['W0'], np.float32)
        scale = np.abs(W).max(1)
        dev64 = float((np.abs(W64 - W).max(1) / scale).max())
        dev32 = float((np.abs(W32 - W).max(1) / scale).max())
        dev64d = float((np.abs(W64d - W).max(1) / scale).max())
        entry = {'fp64_restatement_default_dec_tol_vs_sklearn': dev64d, 'n_train': int(len(train)), 'd': int(X.shape[1]), 'K': int(K), 'C': C, 'fp64_restatement_vs_sklearn': dev64, 'float32_restatement_vs_sklearn': dev32,
                 'fp64_iterations': [i['iterations'] for i in info64], 'fp64_backtracks': [i['backtracks'] for i in info64]}
        assert all(i['converged'] for i in info64), name
        if name in COEFFICIENT_SETS:
            assert dev64 <= 1e-12, (name, dev64)
        if name in R.LINE_SEARCH_SETS:
            assert sum(i['backtracks'] for i in info64) >= 1, name
        if ds['predict']:
            test = R.split(n)[1]
            k = Y[test].sum(1)
            S = R.scores_ref(X[test], W)
            S32 = R.scores_ref(X[test], W32)
            gap = float(R.min_rank_gap(S, k))
            pdev = float(np.abs(1 / (1 + np.exp(-S)) - 1 / (1 + np.exp(-S32))).max())
            assert gap >= 4 * pdev, (name, gap, pdev)
            pred = R.topk_ref(S, k)
            ovr = OneVsRestClassifier(LogisticRegression(max_iter=1000)).fit(Xt, Yt)
            pred_default = R.topk_ref(ovr.decision_function(X[test].astype(np.float64)), k)
            assert np.array_equal(pred, pred_default), name
            tp, fp, fn, exact = R.counts_ref(pred, Y[test])
            entry.update({'n_test': int(len(test)), 'min_probability_gap': gap, 'float32_probability_deviation': pdev,
                          'micro': float(f1_score(Y[test], pred, average='micro')), 'macro': float(f1_score(Y[test], pred, average='macro')),
                          'accuracy': float(accuracy_score(Y[test], pred)), 'default_settings_identical': True,
                          'tp': tp.tolist(), 'fp': fp.tolist(), 'fn': fn.tolist(), 'exact': exact})
        arrays['W_' + name] = W
        report['sets'][name] = entry
        print(name, json.dumps(entry))
    np.savez(os.path.join(GOLDEN, 'nc_ref.npz'), **arrays)
    with open(os.path.join(GOLDEN, 'nc_ref.json'), 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
