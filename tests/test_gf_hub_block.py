"""CPU tests of GF's blocked hub-row arithmetic (gemhip_gf_plan_set_hub_block, DESIGN.md "GF: blocked hub rows"): the device-free part of
gem_amd/csrc/gf_plan.hip as plain C++ behind scripts/asan/gf_hub_block_driver.cpp -- the block size of every width and the table of powers of
a = 1 - eta * regu --, the blocked recurrence restated in numpy fp64 with that table against the sequential fp64 loop, and the plugin's refusal
of hub_block=True with n_gpus > 1.  No HIP, no library, no device."""
import os
import subprocess

import numpy as np
import pytest

import oracle
from gem_amd import build
from gem_amd.embedding.gf import GraphFactorization
from gem_amd.graph import EdgeListGraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SETTINGS = [(1e-4, 1.0), (0.05, 0.01), (0.02, 0.0), (1e-2, 1e-2)]


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc_dir = os.path.dirname(os.path.realpath(build.HIPCC))
    cxx = next(c for c in (os.path.join(hipcc_dir, '..', 'lib', 'llvm', 'bin', 'clang++'), os.path.join(hipcc_dir, 'clang++'), os.path.join(hipcc_dir, 'amdclang++'))
               if os.path.exists(c))
    exe = str(tmp_path_factory.mktemp('gf_hub_block') / 'gf_hub_block_driver')
    subprocess.check_call([cxx, '-std=c++17', '-O2', '-Wall', '-Werror', '-x', 'c++', os.path.join(ROOT, 'gem_amd', 'csrc', 'gf_plan.hip'),
                           os.path.join(ROOT, 'scripts', 'asan', 'gf_hub_block_driver.cpp'), '-o', exe])
    return exe


def block_sizes(driver, widths):
    out = subprocess.check_output([driver, 'block'] + [str(d) for d in widths]).decode().split()
    rows = np.array(out, dtype=np.int64).reshape(-1, 3)
    assert list(rows[:, 0]) == list(widths)
    return {int(d): (int(rw), int(b)) for d, rw, b in rows}


def decay_table(driver, eta, regu, B):
    """(hi, lo) as float32 arrays of B + 1 entries"""
    out = subprocess.check_output([driver, 'decay', '%.9g' % np.float32(eta), '%.9g' % np.float32(regu), str(B)]).decode().split()
    rows = np.array(out, dtype=np.uint64).reshape(-1, 3)
    assert list(rows[:, 0]) == list(range(B + 1))
    return rows[:, 1].astype(np.uint32).view(np.float32), rows[:, 2].astype(np.uint32).view(np.float32)


def test_block_size_of_every_width_and_exact_powers(driver):
    """Every width the GF dispatch supports (even d <= 1024, odd d <= 512) has a block size, the staged row is the dispatch's (a lane holds 2 floats of an
    even width, 1 of an odd one, in 1, 2, 4 or 8 chunks of 64 lanes), no other width has one; and for every block size the rule returns hi[k] + lo[k]
    is a^k to 2^-46, with a^0 = 1 exactly."""
    widths = list(range(1, 1030)) + [2048]
    got = block_sizes(driver, widths)
    sizes = set()
    for d in widths:
        rw, b = got[d]
        if (d % 2 == 0 and d <= 1024) or (d % 2 == 1 and d <= 512):
            per_lane = 2 if d % 2 == 0 else 1
            chunks = -(-d // (64 * per_lane))
            assert rw == 64 * per_lane * next(c for c in (1, 2, 4, 8) if c >= chunks), d
            assert b in (16, 32) and 64 % b == 0, d
            sizes.add(b)
        else:
            assert (rw, b) == (0, 0), d
    assert got[128][1] >= got[1024][1]                      # wide rows may get a smaller block, never a larger one
    for eta, regu in SETTINGS:
        a = 1.0 - float(np.float32(eta)) * float(np.float32(regu))
        for B in sorted(sizes):
            hi, lo = decay_table(driver, eta, regu, B)
            assert hi[0] == 1.0 and lo[0] == 0.0
            want = a ** np.arange(B + 1, dtype=np.float64)
            got_pow = hi.astype(np.float64) + lo.astype(np.float64)
            assert np.all(np.abs(got_pow - want) <= 2.0 ** -46 * want), (eta, regu, B)
            assert np.array_equal(hi, want.astype(np.float32))                   # hi is the fp32 nearest to a^k, not a product of fp32 factors


def blocked_row_f64(x0, Y, w, eta, regu, B, pw):
    """One pass over a row's edges (neighbour rows Y[t], weights w[t]) B at a time, as gf_hub_block_kernel does it, in fp64: p = Y x_0, the B-step
    substitution on r_v = x_t . y_v with G = Y Y^T (no dot product inside it), then x_m = a^m x_0 + sum_u eta a^(m-1-u) s_u y_u; pw[k] = a^k."""
    x = np.array(x0, dtype=np.float64)
    el = eta * regu
    for b0 in range(0, len(w), B):
        Yb, wb = Y[b0:b0 + B], w[b0:b0 + B]
        m = len(wb)
        G = Yb @ Yb.T
        r = Yb @ x
        s = np.zeros(m)
        for u in range(m):
            s[u] = wb[u] - r[u]
            r = r - el * r + eta * s[u] * G[:, u]
        c = eta * s * pw[m - 1 - np.arange(m)]
        x = pw[m] * x + c @ Yb
    return x


def test_blocked_recurrence_equals_the_sequential_loop_in_fp64(driver):
    """A 3000-edge row at d = 16 (93 full blocks and a partial one at B = 32), one neighbour listed twice, weights of both signs and zero: the blocked form
    with the driver's table is the sequential loop of gf.py:93-100 to rounding (1e-12 of the row's scale), for every hyper-parameter setting."""
    d, m, n = 16, 3000, 3200
    B = block_sizes(driver, [d])[d][1]
    assert m % B != 0
    rs = np.random.RandomState(4)
    dst = rs.permutation(np.arange(1, n))[:m].astype(np.int32)
    dst[1700] = dst[11]                                       # the same neighbour twice, in different blocks
    src = np.zeros(m, np.int32)
    w = rs.randn(m)
    w[::7] = 0.0
    X0 = 0.3 * rs.randn(n, d)
    for eta, regu in SETTINGS:
        eta64, regu64 = float(np.float32(eta)), float(np.float32(regu))
        hi, lo = decay_table(driver, eta, regu, B)
        pw = hi.astype(np.float64) + lo.astype(np.float64)
        sweeps = 3
        ref = oracle.gf_train_f64(n, src, dst, w, d, eta64, regu64, sweeps, X0)
        assert np.array_equal(ref[1:], X0[1:])                                   # only row 0 fires
        x = X0[0]
        for _ in range(sweeps):
            x = blocked_row_f64(x, X0[dst], w, eta64, regu64, B, pw)
        scale = float(np.abs(ref[0]).max())
        assert float(np.abs(x - ref[0]).max()) <= 1e-12 * scale, (eta, regu)
        assert float(np.abs(ref[0] - X0[0]).max()) > 1e-3 * scale                # the row moved: the comparison is not of two untouched rows


def test_hub_block_with_several_gpus_is_refused_before_any_device_call():
    """hub_block=True is a per-plan switch of the single-GPU staged path; the N-GPU driver creates its own plans, which GEMHIP_GF_HUB_BLOCK=1 reaches"""
    g = EdgeListGraph(4, np.array([0, 1, 2], np.int32), np.array([1, 2, 3], np.int32))
    with pytest.raises(ValueError, match='GEMHIP_GF_HUB_BLOCK'):
        GraphFactorization(d=4, max_iter=1, eta=0.1, regu=0.1, hub_block=True, n_gpus=2).learn_embedding(graph=g)
