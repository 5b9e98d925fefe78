"""Writes tests/golden/clustering_ref.json / .npz (tests/README_clustering.md).  CPU, sklearn 1.7.2.

    python scripts/make_golden_clustering.py

Per data set of tests/clustering_refs.py: sklearn's KMeans(init=C0, n_init=1, algorithm='lloyd') labels, centres, inertia and n_iter_ at
tol = 0 and tol = 1e-4 on the float32-rounded X passed as float64, and for the SBM sets the metric values of sklearn.metrics.  The script
ASSERTS what the GPU tests rest on: (a) the restatement equals sklearn -- labels and iterations exactly, centres to one fp32 rounding;
(b) no (row, iteration) pair of a set has its two best scores within 2 B; (c) the two relocation sets relocate (in their second
iteration) and no other set does; (d) on the seeding sets the fp64 and float32 restatements choose the same rows and every draw lies at
least 1e-5 of the total from a cumulative boundary."""
import json
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import clustering_refs as R          # noqa: E402

TOLS = (('tol0', 0.0), ('tol1e-4', 1e-4))


def main():
    import sklearn
    from sklearn.cluster import KMeans
    from sklearn.metrics import adjusted_rand_score, homogeneity_score, normalized_mutual_info_score
    meta = {'sklearn': sklearn.__version__, 'sets': {}, 'seeding': {}}
    arrays = {}
    for name, ds in R.data_sets().items():
        X, K, C0 = ds['X'], ds['K'], ds['C0']
        entry = {'K': K, 'seed': ds['seed'], 'n': int(X.shape[0]), 'd': int(X.shape[1])}
        for tag, tol in TOLS:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                sk = KMeans(n_clusters=K, init=C0.astype(np.float64), n_init=1, algorithm='lloyd', tol=tol, max_iter=300).fit(X.astype(np.float64))
            ref = R.lloyd(X, C0, tol=tol, max_iter=300)
            ref32 = R.lloyd(X, C0, tol=tol, max_iter=300, dtype=np.float32)
            assert np.array_equal(ref['labels'], sk.labels_) and ref['n_iter'] == sk.n_iter_, (name, tag, ref['n_iter'], sk.n_iter_)             # (a)
            c32 = sk.cluster_centers_.astype(np.float32)
            ulp = np.spacing(np.abs(c32))
            worst = float((np.abs(c32.astype(np.float64) - ref['centres'].astype(np.float64)) / ulp).max())
            assert worst <= 1.0, (name, tag, worst)
            assert abs(ref['inertia'] - sk.inertia_) <= 1e-9 * sk.inertia_, (name, tag)
            assert ref['tight'] == 0, (name, tag, ref['tight'])                                                                                 # (b)
            assert np.array_equal(ref32['labels'], ref['labels']) and ref32['n_iter'] == ref['n_iter'], (name, tag)
            if name in R.RELOCATION_SETS:
                assert ref['relocated'] and ref['relocated'][0][0] == 2, (name, tag)                                                                # (c)
            else:
                assert not ref['relocated'], (name, tag)
            entry[tag] = {'n_iter': int(sk.n_iter_), 'inertia': float(sk.inertia_), 'strict': bool(ref['strict']), 'pairs': ref['pairs'], 'tight': ref['tight'],
                          'relocated': [[it, rows] for it, rows in ref['relocated']], 'centre_ulp_vs_sklearn': worst}
            arrays['labels_%s_%s' % (name, tag)] = sk.labels_.astype(np.int32)
            arrays['centres_%s_%s' % (name, tag)] = sk.cluster_centers_
            if ds['labels_true'] is not None and tag == 'tol1e-4':
                lt = ds['labels_true']
                table = R.contingency_ref(sk.labels_, lt, K, int(lt.max()) + 1)
                nmi, ari, purity = R.scores_ref(table)
                sk_nmi = float(normalized_mutual_info_score(lt, sk.labels_)); sk_ari = float(adjusted_rand_score(lt, sk.labels_))
                assert abs(nmi - sk_nmi) <= 1e-12 and abs(ari - sk_ari) <= 1e-12, (name, nmi, sk_nmi, ari, sk_ari)
                entry['scores'] = {'nmi': sk_nmi, 'ari': sk_ari, 'purity': purity, 'homogeneity': float(homogeneity_score(lt, sk.labels_)),
                                   'table': table.tolist()}
        meta['sets'][name] = entry
        print(name, json.dumps({k: v for k, v in entry.items() if k != 'scores'}))
    for name, ds in R.seed_sets().items():                                                                                                     # (d)
        rows64, margin = R.seed_pp_ref(ds['X'], ds['K'], ds['u'])
        rows32, margin32 = R.seed_pp_ref(ds['X'], ds['K'], ds['u'], dtype=np.float32)
        assert np.array_equal(rows64, rows32), (name, rows64, rows32)
        assert min(margin, margin32) >= 1e-5, (name, margin, margin32)
        assert len(set(rows64.tolist())) == ds['K'], name
        meta['seeding'][name] = {'K': ds['K'], 'trials': int(ds['u'].shape[1]), 'margin': min(margin, margin32)}
        arrays['seed_rows_%s' % name] = rows64
        print(name, rows64.tolist(), 'margin %.2e' % min(margin, margin32))
    with open(os.path.join(R.GOLDEN, 'clustering_ref.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write('\n')
    np.savez_compressed(os.path.join(R.GOLDEN, 'clustering_ref.npz'), **arrays)


if __name__ == '__main__':
    main()
