"""CPU tests of the host arithmetic of HOPE / Laplacian Eigenmaps / LLE (gem_amd/csrc/hope_host.hip) as plain C++ behind
scripts/asan/hope_host_driver.cpp: no HIP, no library, no device.

Integer decisions (columns kept, q, m, lock counts, jc, the output permutation, signs, terms, the symmetric flag, the transposed row_ptr / col) must
equal what numpy derives; fp64 values must agree with a numpy fp64 evaluation of the same formula within 1e-12 of the result's largest magnitude
(not bit for bit: the driver is built by plain clang++, the library by hipcc).  The scheduling rules of the eigen-path are compared with the
functions of the numpy mirror (tests/hope_sym_mirror.py) for the Katz map, which is the kind the mirror has; for the other two kinds with the
mirror's cycle plan on the shifted spectrum and with the formulas of sym_filter_svd's header comment."""
import math
import os
import subprocess

import numpy as np
import pytest

from gem_amd import build
import hope_sym_mirror as mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    d = tmp_path_factory.mktemp('hope_host')
    exe = str(d / 'hope_host_driver')
    csrc = os.path.join(ROOT, 'gem_amd', 'csrc')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(csrc, 'hope_host.hip'), os.path.join(csrc, 'sym_eig.hip'),
                           os.path.join(ROOT, 'scripts', 'asan', 'hope_host_driver.cpp'), '-lpthread', '-o', exe])

    def run(group, *arrays):
        with open(d / 'in', 'wb') as f:
            for a in arrays:
                a = np.ascontiguousarray(np.asarray(a, np.float64).ravel())
                np.array([a.size], np.float64).tofile(f); a.tofile(f)
        subprocess.check_call([exe, group, str(d / 'in'), str(d / 'out')])
        raw, out, at = np.fromfile(d / 'out', np.float64), [], 0
        while at < raw.size:
            out.append(raw[at + 1:at + 1 + int(raw[at])]); at += 1 + int(raw[at])
        return out
    run.exe = exe
    return run


def close(got, want):
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max(initial=0.0) <= TOL * max(np.abs(want).max(initial=0.0), 1e-300), np.abs(got - want).max()


def test_self_checks_pass(driver):
    run = subprocess.run([driver.exe, 'self'], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stdout.decode()[-3000:] + run.stderr.decode()[-2000:]


KNOB_DEFAULTS = dict(spmm16=1, spmm16_u=0, colmax2=1, sym=-1, sym_amp=1e4, sym_amp0=1e3, sym_maxdeg=32, sym_fused_rr=1, no_lock=0, fixed_depth=0,
                     host_project=0, debug=0, has_basis_cols=0, basis_cols=0, has_depth_cols=0, depth_cols=0)


@pytest.mark.parametrize('env,changed', [
    ({}, {}),                                                                                   # nothing set: the defaults
    ({'SPMM16': '0'}, dict(spmm16=0)), ({'SPMM16_U': '2'}, dict(spmm16_u=2)), ({'COLMAX2': '0'}, dict(colmax2=0)),     # each variable alone
    ({'SYM': '0'}, dict(sym=0)), ({'SYM': '1'}, dict(sym=1)), ({'SYM': '5'}, dict(sym=1)),     # tri-state: unset (-1), 0, non-zero
    ({'SYM_AMP': '250.5'}, dict(sym_amp=250.5)), ({'SYM_AMP': '3'}, dict(sym_amp=10.0)),       # ... and the clamps
    ({'SYM_AMP0': '30'}, dict(sym_amp0=30.0)), ({'SYM_AMP0': '3'}, dict(sym_amp0=10.0)),
    ({'SYM_MAXDEG': '12'}, dict(sym_maxdeg=12)), ({'SYM_MAXDEG': '1'}, dict(sym_maxdeg=2)),
    ({'SYM_FUSED_RR': '0'}, dict(sym_fused_rr=0)), ({'SYM_FUSED_RR': '1'}, {}),
    ({'NO_LOCK': '1'}, dict(no_lock=1)), ({'FIXED_DEPTH': '1'}, dict(fixed_depth=1)), ({'HOST_PROJECT': '1'}, dict(host_project=1)), ({'DEBUG': '1'}, dict(debug=1)),
    ({'NO_LOCK': ''}, dict(no_lock=1)), ({'FIXED_DEPTH': ''}, dict(fixed_depth=1)), ({'HOST_PROJECT': ''}, dict(host_project=1)), ({'DEBUG': ''}, dict(debug=1)),
    ({'NO_LOCK': '0'}, dict(no_lock=1)),                                                        # on by presence, whatever the value
    ({'BASIS_COLS': '700'}, dict(has_basis_cols=1, basis_cols=700)), ({'DEPTH_COLS': '64'}, dict(has_depth_cols=1, depth_cols=64)),
    ({'SPMM16': '0', 'SPMM16_U': '4', 'SYM': '1', 'SYM_AMP': '100', 'DEBUG': '', 'DEPTH_COLS': '48'},
     dict(spmm16=0, spmm16_u=4, sym=1, sym_amp=100.0, debug=1, has_depth_cols=1, depth_cols=48)),
])
def test_knobs_from_a_table(driver, tmp_path, env, changed):
    """hope_knobs_from_env over a lookup table (never the process environment): the fourteen GEMHIP_HOPE_* variables, their defaults and clamps"""
    out = str(tmp_path / 'knobs')
    subprocess.check_call([driver.exe, 'knobs', out] + ['GEMHIP_HOPE_%s=%s' % kv for kv in env.items()], env={'GEMHIP_HOPE_SPMM16': '0', 'GEMHIP_HOPE_DEBUG': '1'})
    raw = np.fromfile(out, np.float64)
    assert raw[0] == len(KNOB_DEFAULTS) == raw.size - 1
    assert dict(zip(KNOB_DEFAULTS, raw[1:])) == dict(KNOB_DEFAULTS, **changed)


def chol_coef(G):
    return np.linalg.inv(np.linalg.cholesky(G).T)


@pytest.mark.parametrize('b', [2, 7, 40])
def test_dense_steps_on_a_full_rank_block(driver, b):
    rs = np.random.RandomState(b)
    Y = rs.randn(5 * b + 3, b) * np.linspace(1.0, 30.0, b)             # columns of different length
    G, H = Y.T @ Y, rs.randn(b, b)
    o = driver('dense', [b, 1e-10, 0.0], G, H)
    assert list(o[0]) == [b, 0] and o[2][0] == b and o[4][0] == 1 and o[9][0] == 1
    close(o[10].reshape(b, b), chol_coef(G))                              # chol_inverse
    C = o[1].reshape(b, b)                                                # orth_pass: the same Cholesky under its pivot floor
    close(C, chol_coef(G)); close(C.T @ G @ C, np.eye(b))
    d = 1.0 / np.sqrt(np.diag(G))
    close(o[7], d); close(o[8].reshape(b, b), G * d[:, None] * d[None, :])
    Cs = chol_coef(G * d[:, None] * d[None, :]) * d[:, None]              # orth_scaled_pass, rr_project: through the normalised Gram matrix
    close(o[3].reshape(b, b), Cs); close(o[5].reshape(b, b), Cs)
    close(o[3].reshape(b, b).T @ G @ o[3].reshape(b, b), np.eye(b))
    close(o[6].reshape(b, b), Cs.T @ (0.5 * (H + H.T)) @ Cs)             # Hq = C2^T sym(H) C2


@pytest.mark.parametrize('b', [2, 9])
def test_dense_steps_fall_back_on_rank_loss(driver, b):
    rs = np.random.RandomState(10 + b)
    Y = rs.randn(4 * b + 5, b)
    H = rs.randn(b, b)
    for case in ('repeated column', 'null column'):
        Yc = Y.copy()
        Yc[:, b - 1] = Yc[:, 0] if case == 'repeated column' else 0.0
        G = Yc.T @ Yc
        o = driver('dense', [b, 1e-10, 0.0], G, H)
        assert list(o[0]) == [b - 1, 1], case                             # orth_pass: fallback ("remixed"), one direction dropped
        assert o[2][0] == b - 1 and o[4][0] == 0 and o[5].size == 0, case
        assert np.array_equal(o[6], H.ravel()), case                      # rr_project refused: H as it was
        w, Z = np.linalg.eigh(G)
        top = Z[:, 1:] / np.sqrt(w[1:])
        C = o[1].reshape(b, b - 1)
        close(C.T @ G @ C, np.eye(b - 1)); close(C @ C.T, top @ top.T)    # (C C^T: free of the eigenvectors' signs)
        d = np.where(np.diag(G) > 0, 1.0 / np.sqrt(np.where(np.diag(G) > 0, np.diag(G), 1.0)), 0.0)
        close(o[7], d)
        ws, Zs = np.linalg.eigh(G * d[:, None] * d[None, :])
        tops = (Zs[:, 1:] / np.sqrt(ws[1:])) * d[:, None]
        Cs = o[3].reshape(b, b - 1)
        close(Cs.T @ G @ Cs, np.eye(b - 1)); close(Cs @ Cs.T, tops @ tops.T)


@pytest.mark.parametrize('kind,beta', [(0, 0.3), (0, -0.3), (1, 1.0), (2, 2.5)])
def test_ritz_order(driver, kind, beta):
    ma = 12
    rs = np.random.RandomState(kind)
    M = rs.randn(ma, ma)
    ev, Z = np.linalg.eigh(0.5 * (M + M.T))
    f = {0: lambda x: beta * x / (1.0 - beta * x), 1: lambda x: 1.0 + x, 2: lambda x: beta - x}[kind]
    order = np.argsort(-np.abs(f(ev)), kind='stable')
    for C2 in (np.zeros(0), np.triu(rs.randn(ma, ma))):
        th, C, Ct, S, fe = driver('ritz', [ma, kind, beta], Z, ev, C2, M)
        assert np.array_equal(th, ev[order])                              # the permutation, exactly
        want = Z[:, order] if C2.size == 0 else C2 @ Z[:, order]
        close(C.reshape(ma, ma), want); close(Ct.reshape(ma, ma), -want * ev[order])
        close(S.reshape(ma, ma), 0.5 * (M + M.T)); close(fe, f(ev))


def sym_inputs(kind, rs):
    """A spectrum, a Ritz block sorted by |f| and residuals, as a cycle of the eigen-path sees them"""
    beta = {0: 0.04, 1: 1.0, 2: 1.9}[kind]
    br = 0.7
    L = {0: br / abs(beta), 1: 1.0001, 2: beta}[kind]
    f = {0: lambda x: mirror.katz_f(beta, x), 1: lambda x: 1.0 + x, 2: lambda x: beta - x}[kind]
    th = (rs.rand(24) if kind == 2 else rs.rand(24) * 2 - 1) * 0.95 * L
    th = th[np.argsort(-np.abs(f(th)), kind='stable')]
    res = np.abs(th) * 10.0 ** rs.uniform(-6, -1, th.size) * np.linspace(0.01, 1.0, th.size)
    return beta, br, L, f, th, res


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_eigen_path_rules_match_the_mirror(driver, kind):
    rs = np.random.RandomState(100 + kind)
    for trial in range(40):
        beta, br, L, f, th, res = sym_inputs(kind, rs)
        smin = 0.0 if kind == 2 else -L
        res_floor = 0.25 * L if kind == 2 else 0.0
        nl, cyc = int(rs.choice([0, 0, 3, 11])), int(rs.choice([0, 1, 7]))
        want, b_min, tol = int(rs.choice([1, 2, 8, 16])), int(rs.choice([2, 10, 30])), float(rs.choice([1e-5, 1e-3, 1e-14]))
        amp, amp0, max_degree = float(rs.choice([1e4, 30.0])), 1e3, int(rs.choice([32, 6]))
        tau_prev = float(rs.choice([0.0, 0.3, 5.0]))
        lo = smin + rs.rand() * 0.3 * L
        hi = lo + (0.2 + rs.rand()) * 0.5 * L
        spec, cy, lock, nxt = driver('sym', [kind, beta, br, lo, hi, nl, cyc, amp, amp0, max_degree, want, b_min, tol, tau_prev], th, res)
        close(spec, [L, smin, L, res_floor, 0.25 * L if kind == 2 else -L, L if kind == 2 else 0.5 * L])
        # the cycle plan depends on distances inside the spectrum only: the mirror's rule for [-L', L'] on the shifted values
        mid = 0.5 * (smin + L)
        c, e, q, m = mirror.cycle_plan(lo - mid, hi - mid, L - mid, th - mid, nl, cyc, amp, amp0, max_degree)
        assert (cy[2], cy[3]) == (q, m), (trial, cy, q, m)
        close(cy[:2], [c + mid, e])
        lock_tol = 0.1 * math.sqrt(max(float(np.float32(tol)), 1e-12))
        lead = min(want, th.size)
        close(lock[:1], [(res[:lead] / np.maximum(np.maximum(np.abs(th[:lead]), 1e-3 * L), res_floor)).max()])
        if kind == 0:
            newl = mirror.lock_count(want, b_min, th, res, lock_tol)
        else:
            newl = 0
            while newl < want - 1 and newl < th.size - b_min and res[newl] < lock_tol * max(abs(th[newl]), res_floor):
                newl += 1
        assert lock[1] == newl, trial
        left = th[newl:]
        if kind == 0:
            jc, tau, nlo, nhi = mirror.next_interval(beta, L, want - newl, left, tau_prev)
        else:
            jc = max(0, min(left.size - 1, (want - newl) + (left.size - (want - newl)) // 2 - 1))
            tau = max(tau_prev, abs(f(left[jc])))
            nlo, nhi = (max(beta - tau, 0.01 * L), L) if kind == 2 else (-L, max(min(tau - 1.0, 0.98 * L), -0.5 * L))
        assert nxt[0] == jc, trial
        close(nxt[1:], [tau, nlo, nhi])


def test_eigen_path_locks_leading_pairs_and_resets_the_interval_at_tau_zero(driver):
    """the grid above rarely converges a pair: here three have, and b_min / want decide how many may go; a block whose cut-off column maps to 0
    gets the first interval again"""
    beta, br = 0.04, 0.7
    L = br / beta
    th = np.array([0.9, -0.85, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3]) * L
    res = np.array([1e-9, 1e-9, 1e-9, 1e-2, 1e-2, 1e-2, 1e-2, 1e-2])
    for want, b_min in [(6, 2), (3, 2), (6, 6), (1, 2), (6, 8)]:
        lock = driver('sym', [0, beta, br, -L, 0.5 * L, 0, 1, 1e4, 1e3, 32, want, b_min, 1e-5, 0.0], th, res)[2]
        assert lock[1] == mirror.lock_count(want, b_min, th, res, 0.1 * math.sqrt(float(np.float32(1e-5)))) == max(0, min(3, want - 1, th.size - b_min))
    for kind, beta, zero in [(0, 0.04, 0.0), (1, 1.0, -1.0), (2, 1.9, 1.9)]:
        spec, _, _, nxt = driver('sym', [kind, beta, br, 0.1, 0.2, 0, 1, 1e4, 1e3, 32, 1, 1, 1e-5, 0.0], [zero], [1.0])
        assert list(nxt) == [0, 0.0, spec[4], spec[5]]


def test_block_krylov_rules(driver):
    rs = np.random.RandomState(7)
    for trial in range(40):
        b, ks, n = int(rs.choice([4, 20, 80, 200])), int(rs.choice([1, 5, 8])), int(rs.choice([34, 300, 100000]))
        has_basis, basis = int(rs.rand() < 0.3), int(rs.choice([-5, 0, 100, 700]))
        has_depth, depth = int(rs.rand() < 0.3), int(rs.choice([0, 64, 1000]))
        nl, m0, oversample = int(rs.choice([0, 0, 5, 30])), int(rs.choice([0, 3, 40])), int(rs.choice([0, 1, 16]))
        tol, want = float(rs.choice([1e-5, 1e-14])), int(rs.choice([1, 3, 40]))
        prev_b = int(rs.choice([2, 18, 60]))
        ma, mt = 9, int(rs.choice([1, 4, 9]))
        act = np.sort(rs.rand(prev_b) + 0.1)[::-1] * (rs.rand() < 0.9)
        D = np.diag((act ** 2 * 10.0 ** rs.uniform(-8, -1, prev_b) * np.linspace(0.0, 1.0, prev_b)) ** 2) + np.triu(rs.randn(prev_b, prev_b), 1)
        Zt = rs.randn(mt, ma)                                            # column-major ma x mt
        head, C = driver('krylov', [b, ks, n, has_basis, basis, nl, m0, has_depth, depth, oversample, tol, want, prev_b, mt, ma], act, D, Zt)
        cols = b * (ks + 1) + b * (ks + 1) // 5
        if has_basis:
            cols = max(b * (ks + 1), basis)
        mmax = min(cols, n, 512)
        steps = ks
        if nl > 0 and m0 > 0:
            steps = max(ks, ((min(mmax, max(depth, nl + m0)) if has_depth else mmax) - nl) // m0 - 1)
        b_min = min(b, max(2 * oversample, 16))
        lock_tol = 0.1 * math.sqrt(max(float(np.float32(tol)), 1e-12))
        newl = 0
        while newl < want - 1 and newl < prev_b - b_min and act[newl] > 0 and math.sqrt(max(D[newl, newl], 0.0)) < lock_tol * act[newl] * act[newl]:
            newl += 1
        nb = min(mt, max(b - nl, b_min))
        assert [head[0], head[1], head[2], head[4], head[5]] == [mmax, steps, b_min, newl, nb], trial
        close(head[3:4], [lock_tol])
        assert np.array_equal(C.reshape(ma, nb), Zt[:nb].T)


@pytest.mark.parametrize('has_zt,from_image,unit_v', [(0, 0, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1)])
def test_output_selection(driver, has_zt, from_image, unit_v):
    """both solvers' forms: basis columns with signs (eigen-path), locked columns + Ritz vectors of the active block (block-Krylov path)"""
    rs = np.random.RandomState(3 + 2 * has_zt + unit_v)
    k, nl, ma = 6, 4, 7
    s = np.round(rs.rand(nl + ma) * 8) / 4.0                             # ties and a zero or two among the values
    s[2] = s[7]; s[5] = 0.0
    sgn = rs.choice([-1.0, 1.0], nl + ma) if not has_zt else np.ones(nl + ma)
    cand = np.stack([s, sgn, np.arange(nl + ma)], axis=1)
    Zt = rs.randn(ma, ma)                                                 # column-major ma x ma
    colmax = rs.choice([-0.5, 0.0, 2.0], k)
    sig_old = rs.rand(k)
    o = driver('out', [k, nl, ma, has_zt, from_image, unit_v], s, sig_old, cand, Zt, colmax)
    sig = np.sort(s)[::-1][:k]
    close(o[0], sig); close(o[1], [np.abs(sig - sig_old).max() / sig[0]]); close(o[2], sig)
    order = np.argsort(-s, kind='stable')
    assert np.array_equal(o[9], order)                                    # the output permutation, ties in candidate order
    assert np.array_equal(o[3], s[order[:k]][::-1].astype(np.float32))    # sigma ascending
    Cu, Cv = np.zeros((nl + ma, k)), np.zeros((nl + ma, k))
    for r in range(k):
        j, c, sv = k - 1 - r, order[r], s[order[r]]
        inv = lambda x: 1.0 / x if x > 0 else 0.0
        su = (inv(sv) if unit_v else inv(math.sqrt(sv))) if from_image else sgn[c] * math.sqrt(sv)
        vec = np.eye(nl + ma)[c] if (not has_zt or c < nl) else np.concatenate([np.zeros(nl), Zt[c - nl]])
        Cu[:, j], Cv[:, j] = vec * su, vec * (1.0 if unit_v else math.sqrt(sv))
    close(o[4].reshape(nl + ma, k), Cu); close(o[5].reshape(nl + ma, k), Cv)
    flip = np.where(colmax < 0, -1.0, 1.0)
    assert o[6][0] == float((colmax < 0).any())
    assert np.array_equal(o[7], (o[4].reshape(nl + ma, k) * flip).ravel()) and np.array_equal(o[8], (o[5].reshape(nl + ma, k) * flip).ravel())   # the signs
    assert list(o[10]) == [1.0 * 1e-3, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 0.0, 0.0, 9.0, 10.0 * 1e-3]                                         # stats[] layout


def random_csr(rs, n, symmetric, dups, empty):
    """rows sorted by column; row `empty` (and, if symmetric, its column) without entries; dups: every entry of rows 0..9 twice, with another weight"""
    import scipy.sparse as sp
    A = sp.random(n, n, density=3.0 / n, random_state=rs, format='coo', data_rvs=lambda m: (rs.randint(1, 9, m) / 4.0))
    A = (A + A.T if symmetric else A).tocoo()
    rows, ci, w = A.row.astype(np.int64), A.col.astype(np.int32), A.data.astype(np.float32)
    keep = (rows != empty) & ((ci != empty) | (not symmetric))
    rows, ci, w = rows[keep], ci[keep], w[keep]
    if dups:
        extra = rows < 10
        rows, ci, w = np.concatenate([rows, rows[extra]]), np.concatenate([ci, ci[extra]]), np.concatenate([w, w[extra] + 1.0])
    by = np.lexsort((np.arange(rows.size), ci, rows))
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return rp, rows[by], ci[by], w[by]


@pytest.mark.parametrize('symmetric,dups', [(True, False), (False, False), (False, True)])
def test_csr_setup(driver, symmetric, dups):
    n, k = 300, 5
    rp, rows, ci, w = random_csr(np.random.RandomState(17), n, symmetric, dups, 39)
    nnz = len(ci)
    assert rp[40] == rp[39] and nnz > 2 * n
    for one_weight_off in (False, True):
        wv = w.copy()
        if one_weight_off:
            wv[nnz // 2] += 0.25
        for has_w, br in ((1, 0.5), (0, 0.93)):
            o = driver('csr', [n, nnz, has_w, br, k], rp, ci, wv)
            assert list(o[0]) == [0, -1]
            by = np.argsort(ci, kind='stable')                            # stable counting sort by column
            rpT = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=n))])
            assert np.array_equal(o[1], rpT) and np.array_equal(o[2], rows[by]) and np.array_equal(o[3], wv[by])
            sym = bool(np.array_equal(rpT, rp) and np.array_equal(rows[by], ci) and np.array_equal(wv[by], wv))     # (rows sorted: A^T's arrays are A's)
            assert sym == (symmetric and not one_weight_off)
            assert o[4][0] == sym and o[4][2] == max(1, min(400, math.ceil(math.log(1e-8) / math.log(br))))
            a = np.abs(wv.astype(np.float64))
            close(o[4][1:2], [math.sqrt(np.bincount(rows, a, n).max() * np.bincount(ci, a, n).max())])
            we = wv.astype(np.float64) if has_w else np.ones(nnz)
            deg = np.bincount(rows, we, n)
            dinv = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
            assert np.array_equal(o[5], (dinv[rows] * we * dinv[ci]).astype(np.float32))          # D^-1/2 A D^-1/2, rounded to fp32 once
            l1 = np.bincount(rows, np.abs(we), n)
            assert np.array_equal(o[6], (we / l1[rows]).astype(np.float32))                       # l1-normalised rows
            pad = np.concatenate([wv, np.zeros(-nnz % k, np.float32)]).reshape(-1, k)
            assert np.array_equal(o[7], pad[:, ::-1].ravel())                                     # reverse_columns


def test_csr_refusals_and_an_empty_matrix(driver):
    rp, ci = [0, 2, 3, 3], [1, 2, 0]
    assert list(driver('csr', [3, 3, 0, 0.5, 2], rp, [1, 3, 0], [])[0]) == [3, 1]                 # COLUMN, at entry 1
    assert list(driver('csr', [3, 3, 0, 0.5, 2], rp, [1, -1, 0], [])[0]) == [3, 1]
    assert driver('csr', [3, 2, 0, 0.5, 2], rp, ci, [])[0][0] == 2                                # ROW_PTR
    assert driver('csr', [3, 3, 0, 0.5, 2], [1, 2, 3, 3], ci, [])[0][0] == 2
    assert driver('csr', [1, 0, 0, 0.5, 2], [0, 0], [], [])[0][0] == 1                            # BAD_ARGUMENTS: n < 2
    o = driver('csr', [3, 0, 0, 0.0, 2], [0, 0, 0, 0], [], [])                                    # nnz = 0
    assert list(o[0]) == [0, -1] and list(o[1]) == [0, 0, 0, 0] and o[2].size == 0 and list(o[4]) == [0, 0.0, 1]
