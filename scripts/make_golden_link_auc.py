"""Writes the ranking / link-classification fixtures under tests/golden/ (tests/README_link_auc.md).  CPU only; needs scikit-learn (1.7.2
when the fixtures were made).

    python scripts/make_golden_link_auc.py

link_auc_ref.npz   w_<op> [d + 1] fp64, weights then intercept, per operator: sklearn LogisticRegression(C=1, solver='newton-cholesky',
                   tol=1e-12, max_iter=1000) on the float32 pair features of the fixture's training pairs; roc_* / pr_*: sklearn's roc_curve
                   (drop_intermediate=False) and precision_recall_curve arrays on tests/rank_refs.py curve_set().
link_auc_ref.json  the pair counts; per operator and for 'dot': sklearn's roc_auc_score / average_precision_score of the test pairs' fp64
                   scores, delta, `near` and the AP sensitivity (below); the largest deviation of sklearn's metrics and curve arrays from the
                   exact rationals; the figures the asserted conditions were checked with.

Inputs are NOT stored: rank_refs rebuilds them from hope_sbm1024_d32.npz, sbm1024_edges.npy and seeds.  Asserted here, because the tests rest
on it: (a) per operator the fp64 restatement of the solver (tests/nc_refs.py newton_fit at dec_tol = 1e-12) equals sklearn's coefficients to
1e-12 of max |w*|; (b) per operator and for 'dot', with delta = 4 x the largest score deviation of the float32-restated fit from the fp64 one
(for 'dot': 4 x the fp64 summation bound), the share near / (P N) of (positive, negative) test pairs whose scores lie within delta is at
most 1e-3 -- the end-to-end test allows the AUC to move by exactly that share; (c) no AUC is 0.5 or 1.  The seeds of rank_refs (split 3,
pairs 0) are the first pair tried on which (a) holds for all four operators."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
REFERENCE_DEC_TOL = 1e-12
NEAR_CAP = 1e-3


def main():
    import sklearn
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import average_precision_score, precision_recall_curve, roc_auc_score, roc_curve
    import nc_refs as NR
    import rank_refs as R

    arrays, report = {}, {'sklearn': sklearn.__version__, 'ops': {}}
    X = R.embedding()
    _, _, pairs = R.fixture_pairs()
    for k in ('n_train_pos', 'n_train_neg', 'n_test_pos', 'n_test_neg'):
        report[k] = int(pairs[k])
    st, ed, y = pairs['train']
    tst, ted, ty = pairs['test']
    metric_dev = 0.0

    def record(name, s_ref, delta, extra):
        nonlocal metric_dev
        ex = R.exact_scores(s_ref, ty)
        auc, ap = float(roc_auc_score(ty, s_ref)), float(average_precision_score(ty, s_ref))
        metric_dev = max(metric_dev, abs(auc - float(ex['auc'])), abs(ap - float(ex['ap'])))
        near = R.near_pairs(s_ref, ty, delta)
        share = near / float(ex['P'] * ex['N'])
        assert share <= NEAR_CAP, (name, share)
        assert 0.5 < auc < 1.0, (name, auc)
        entry = {'auc': auc, 'ap': ap, 'delta': float(delta), 'near': near, 'near_share': share, 'ap_sensitivity': R.ap_sensitivity(s_ref, ty, delta),
                 'n_thresholds': ex['T']}
        entry.update(extra)
        report['ops'][name] = entry
        print(name, json.dumps(entry))

    for op in R.OPS:
        F = R.features_ref(op, X, st, ed)
        m = LogisticRegression(C=1.0, solver='newton-cholesky', tol=1e-12, max_iter=1000).fit(F.astype(np.float64), y)
        w = np.append(m.coef_[0], m.intercept_[0])
        w64, info64 = NR.newton_fit(F, y, 1.0, None, np.float64, dec_tol=REFERENCE_DEC_TOL)
        w32, _ = NR.newton_fit(F, y, 1.0, None, np.float32)
        scale = np.abs(w).max()
        dev64 = float(np.abs(w64 - w).max() / scale)
        dev32 = float(np.abs(np.asarray(w32, np.float64) - w).max() / scale)
        assert info64['converged'] and dev64 <= 1e-12, (op, dev64)
        Ft = R.features_ref(op, X, tst, ted)
        s_ref = R.scores_ref(Ft, w)
        delta = 4 * float(np.abs(R.scores_ref(Ft, np.asarray(w32, np.float64)) - R.scores_ref(Ft, w64)).max())
        arrays['w_' + op] = w
        record(op, s_ref, delta, {'fp64_restatement_vs_sklearn': dev64, 'float32_restatement_vs_sklearn': dev32, 'fp64_iterations': info64['iterations']})
    A, B = X[tst].astype(np.float64), X[ted].astype(np.float64)
    s_dot = (A * B).sum(1)
    record('dot', s_dot, 4 * float((4 * (X.shape[1] + 1) * 2.0 ** -53 * (np.abs(A) * np.abs(B)).sum(1)).max()), {})

    s, yc = R.curve_set()
    ex = R.exact_scores(s, yc)
    fpr, tpr, thr = roc_curve(yc, s, drop_intermediate=False)
    prec, rec, pthr = precision_recall_curve(yc, s)
    fr, tr = R.roc_ref(ex)
    pr, rr = R.pr_ref(ex)
    assert len(fpr) == ex['T'] + 1 and len(prec) == ex['T'] + 1
    assert np.array_equal(thr[1:], ex['thr']) and np.array_equal(pthr, ex['thr'][::-1])
    curve_dev = max(R.max_dev(fpr, fr), R.max_dev(tpr, tr), R.max_dev(prec, pr), R.max_dev(rec, rr))
    arrays.update({'roc_fpr': fpr, 'roc_tpr': tpr, 'roc_thr': thr, 'pr_precision': prec, 'pr_recall': rec, 'pr_thr': pthr})
    report['curve'] = {'m': int(len(s)), 'n_thresholds': ex['T'], 'sklearn_vs_exact': curve_dev,
                       'auc': float(roc_auc_score(yc, s)), 'ap': float(average_precision_score(yc, s))}
    for name, (sm, ym) in R.metric_sets().items():
        exm = R.exact_scores(sm, ym)
        metric_dev = max(metric_dev, abs(float(roc_auc_score(ym, sm)) - float(exm['auc'])), abs(float(average_precision_score(ym, sm)) - float(exm['ap'])))
    report['sklearn_metrics_vs_exact'] = metric_dev
    print('curve', json.dumps(report['curve']), 'metrics vs exact', metric_dev)
    np.savez(os.path.join(GOLDEN, 'link_auc_ref.npz'), **arrays)
    with open(os.path.join(GOLDEN, 'link_auc_ref.json'), 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write('\n')


if __name__ == '__main__':
    main()
