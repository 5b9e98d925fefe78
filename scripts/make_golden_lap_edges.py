"""Writes tests/golden/ref_lap_edges.npz (tests/README_lap_lle.md): what the reference's LaplacianEigenmaps.learn_embedding returns on the graphs
of tests/lap_lle_refs.py.  CPU only; needs the reference implementation (the GEM package) -- give its directory as the argument -- and
networkx / scipy (3.4.2 / 1.15.3 when the fixture was made).

    python scripts/make_golden_lap_edges.py <directory of the reference>

weighted_d3, isolated_d3, isolated_d6, tiny_d1, tiny_d2    float64 [n][d]: the embedding, rows in graph.nodes order
The graphs are NOT stored: they are lap_lle_refs.weighted(), isolated() and tiny().to_networkx().  `components` has no golden: a single-vector
ARPACK run is not guaranteed to find a triple eigenvalue.

Every case runs in an interpreter of its own, as the first eigs() call of its process.  ARPACK draws its start vector from a generator that
lives as long as the process, and on `tiny` (n = 6: the Krylov space is the whole space, so the zero-degree node 4 is found at networkx's
eigenvalue 0 next to the trivial vector) the answer depends on it.  In the first call e_4 sorts first and is the column that is dropped: the
embedding is [D^1/2 1, next vectors], inside the span of the fp64 vectors, with a zero row at node 4.  Later calls of the same process return
e_4 as the embedding's first column for some d (measured for the d sequences 1 1 1 2 2 and 2 2 1 2 1: the first call in the span to 1e-15, three
of the four later ones at distance 1).  `weighted` and `isolated` do not depend on it (ten calls in one process: 4e-14 at most)."""
import contextlib
import io
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (('weighted', 3), ('isolated', 3), ('isolated', 6), ('tiny', 1), ('tiny', 2))


def one(reference_dir, name, d, path):
    sys.path[:0] = [reference_dir, ROOT, os.path.join(ROOT, 'tests')]
    import gem.embedding.lap
    assert not os.path.abspath(gem.embedding.lap.__file__).startswith(ROOT + os.sep), 'this is the drop-in package of this repository, not the reference'
    import lap_lle_refs as refs
    G = refs.case_graph(name)
    with contextlib.redirect_stdout(io.StringIO()):          # (it prints its reconstruction error)
        Y = gem.embedding.lap.LaplacianEigenmaps(d=d).learn_embedding(graph=G, is_weighted=True, no_python=True)
    Y = np.asarray(Y, dtype=np.float64)
    assert Y.shape == (len(G), d)
    ref = refs.reference('lap', name)
    print('%s d=%d: distance from the fp64 span of the first %d vectors %.2e, zero-degree rows max %.1e'
          % (name, d, d + 1, refs.span_distance(ref, Y, d + 1), np.abs(Y[ref.zero_degree]).max() if ref.zero_degree else 0.0), flush=True)
    np.save(path, Y)


def main():
    if len(sys.argv) == 6 and sys.argv[1] == '--one':
        return one(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
    reference_dir = os.path.abspath(sys.argv[1])
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, d in CASES:
            path = os.path.join(tmp, '%s_d%d.npy' % (name, d))
            subprocess.run([sys.executable, os.path.abspath(__file__), '--one', reference_dir, name, str(d), path], check=True)
            out['%s_d%d' % (name, d)] = np.load(path)
    np.savez_compressed(os.path.join(ROOT, 'tests', 'golden', 'ref_lap_edges.npz'), **out)


if __name__ == '__main__':
    sys.exit(main())
