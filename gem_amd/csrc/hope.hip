// hope.hip -- HOPE (Katz-proximity truncated SVD) for MI355X (gfx950).
//
// Replaces gem/embedding/hope.py:28-36:
//     A  = nx.to_numpy_matrix(graph)                    dense n x n, rows in graph.nodes order
//     S  = inv(I - beta A) . (beta A)                   dense O(n^3)
//     u, s, vt = scipy.sparse.linalg.svds(S, k=d//2)    ARPACK, s ascending
//     X  = [u sqrt(s) | vt.T sqrt(s)]
// S is never formed here.  S = sum_{t>=1} (beta A)^t, so S.Y and S^T.Y are fixed-point iterations of
// CSR SpMMs (Z <- W + beta A Z), HBM-bound; the top-k singular triplets come from a restarted
// randomized BLOCK KRYLOV method on S^T S with full re-orthogonalisation and a Rayleigh-Ritz step.
// The dense tall-skinny products it needs -- Gram matrices X^T Y and basis updates X.C -- run on the
// matrix cores with the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32); the tiny projected eigenproblems
// (<= 512 x 512) are solved on the host in fp64 (Householder tridiagonalisation + implicit QL).
//
// Kernels and what bounds them (n rows, b block columns, m basis columns):
//   hope_spmm_kernel    Y = alpha A X (+W)    HBM/MALL: nnz*(8 + 4b) gather + 8 n b      [dominant]
//   hope_gram_kernel    P = X^T Y per slab    MFMA fp32 (2 n m1 m2 flop), operands stream from L2
//   hope_tsgemm_kernel  O = S + a X C         MFMA fp32 (2 n m b flop)
#include "common.hpp"
#include "hope_host.hpp"
#include "sym_eig.hpp"
#include <vector>
#include <cmath>
#include <algorithm>
#include <chrono>
#include <cstdlib>

using namespace gemhip;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ SpMM (CSR)
// One wavefront per row; lane l owns columns l, l+64, ... of the dense block (a neighbour row of
// the block is one contiguous 4b-byte read).  (col,val) pairs are read 64 at a time, coalesced,
// and broadcast with v_readlane; four neighbour rows are kept in flight.
template <int CPL>
__global__ __launch_bounds__(256) void hope_spmm_kernel(int64_t n, const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                        const float *__restrict__ val, float alpha, const float *__restrict__ X, int ldx,
                                                        const float *__restrict__ Wadd, int ldw, float *__restrict__ Y, int ldy, int b,
                                                        float wa, const float *__restrict__ W2, int ldw2, float wb)
{
    const int lane = lane_id();
    const int64_t i = xcd_contiguous_block(blockIdx.x, gridDim.x) * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
    float acc[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) acc[c] = 0.f;
    for (int64_t e = e0; e < e1; e += WAVE) {
        const int cnt = (int)((e1 - e) < (int64_t)WAVE ? (e1 - e) : (int64_t)WAVE);
        const int32_t cj = lane < cnt ? col[e + lane] : 0;
        const float vj = lane < cnt ? val[e + lane] : 0.f;
        for (int k = 0; k < cnt; k += 4) {
            float xr[4][CPL];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int kk = (k + u) < cnt ? (k + u) : (cnt - 1);
                const float *px = X + (int64_t)bcast_lane(cj, kk) * ldx;
#pragma unroll
                for (int c = 0; c < CPL; ++c) { const int cc = lane + c * WAVE; xr[u][c] = cc < b ? px[cc] : 0.f; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float v = (k + u) < cnt ? bcast_lane(vj, (k + u) < cnt ? (k + u) : 0) : 0.f;
#pragma unroll
                for (int c = 0; c < CPL; ++c) acc[c] += v * xr[u][c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
        const int cc = lane + c * WAVE;
        if (cc >= b) continue;
        if (!W2 && wa == 1.0f) Y[i * ldy + cc] = alpha * acc[c] + (Wadd ? Wadd[i * ldw + cc] : 0.f);
        else                                                    // three-term recurrences: alpha A X + wa W + wb W2
            Y[i * ldy + cc] = fmaf(alpha, acc[c], fmaf(wa, Wadd ? Wadd[i * ldw + cc] : 0.f, W2 ? wb * W2[i * ldw2 + cc] : 0.f));
    }
}

// Quarter-wave variant for blocks of up to 128 columns: 16 lanes per row, four rows per wavefront.  The one-row-per-wavefront kernel
// above is bound by its dependent chain (row_ptr -> col/val -> gathers -> store: ~12 rounds of resident waves at n = 100k, each a few
// microseconds) and leaves the lanes beyond b idle; four independent chains per wavefront cut the rounds by four.  Lane l of a group
// owns columns l, l+16, ...: a neighbour's row is read as CPL16 64-byte segments.  Neighbours are added in edge order like above: the same order,
// not the same bits -- the compiler fuses the kernel above's multiply-adds and compiles this one's to packed multiplies and adds, so the two
// agree to rounding, while every U of this kernel gives the same bits (tests/test_hope_blocks_gpu.py::test_spmm_variants_are_bit_identical).
template <int CPL16, int U>
__global__ __launch_bounds__(256) void hope_spmm16_kernel(int64_t n, const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                          const float *__restrict__ val, float alpha, const float *__restrict__ X, int ldx,
                                                          const float *__restrict__ Wadd, int ldw, float *__restrict__ Y, int ldy, int b,
                                                          float wa, const float *__restrict__ W2, int ldw2, float wb)
{
    const int l16 = threadIdx.x & 15;
    const int64_t i = xcd_contiguous_block(blockIdx.x, gridDim.x) * 16 + (threadIdx.x >> 4);
    if (i >= n) return;
    const int64_t e0 = row_ptr[i], e1 = row_ptr[i + 1];
    // Round 5: the row's dependent chain is row_ptr -> (column, value) -> gathers -> addends -> store, and at SBM 100k/1M a launch is only ~3 rounds of
    // resident wavefronts deep, so the chain IS the launch time.  Two links go: (1) the addends of the epilogue (the recurrence's W1 / W2 terms) are
    // requested here, before the neighbour loop, instead of after it; (2) lane k of the 16-lane group fetches the (column, value) pair of the row's k-th
    // neighbour -- ONE coalesced request for up to 16 neighbours instead of one round trip per U of them -- and the group reads them back with
    // ds_bpermute, so that every gather of a row of <= 16 neighbours can be in flight U at a time with nothing but arithmetic between the rounds.
    // Same products, same order of the additions: bit-identical to the round-4 kernel.
    float wadd[CPL16], w2v[CPL16];
#pragma unroll
    for (int c = 0; c < CPL16; ++c) {
        const int cc = l16 + c * 16;
        wadd[c] = (Wadd && cc < b) ? Wadd[i * ldw + cc] : 0.f;
        w2v[c] = (W2 && cc < b) ? W2[i * ldw2 + cc] : 0.f;
    }
    float acc[CPL16];
#pragma unroll
    for (int c = 0; c < CPL16; ++c) acc[c] = 0.f;
    int32_t cl = 0; float vl = 0.f;
    if (e0 + l16 < e1) { cl = col[e0 + l16]; vl = val[e0 + l16]; }
    for (int64_t e = e0; e < e1; e += 16) {
        const int32_t c_cur = cl; const float v_cur = vl;
        if (e + 16 + l16 < e1) { cl = col[e + 16 + l16]; vl = val[e + 16 + l16]; }          // the next 16 neighbours travel while these are gathered
        const int cnt = (int)((e1 - e) < 16 ? (e1 - e) : 16);
        for (int k = 0; k < cnt; k += U) {
            float xr[U][CPL16], vj[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int kk = (k + u) < cnt ? (k + u) : (cnt - 1);
                const int32_t cj = __shfl(c_cur, kk, 16);
                const float vv = __shfl(v_cur, kk, 16);
                vj[u] = (k + u) < cnt ? vv : 0.f;
                const float *px = X + (int64_t)cj * ldx;
#pragma unroll
                for (int c = 0; c < CPL16; ++c) { const int cc = l16 + c * 16; xr[u][c] = cc < b ? px[cc] : 0.f; }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < CPL16; ++c) acc[c] += vj[u] * xr[u][c];
        }
    }
#pragma unroll
    for (int c = 0; c < CPL16; ++c) {
        const int cc = l16 + c * 16;
        if (cc >= b) continue;
        if (!W2 && wa == 1.0f) Y[i * ldy + cc] = alpha * acc[c] + wadd[c];
        else Y[i * ldy + cc] = fmaf(alpha, acc[c], fmaf(wa, wadd[c], W2 ? wb * w2v[c] : 0.f));
        // (measured and dropped, round 4: reading W2 -- the oldest term of the three-term recurrence, its last use -- with the non-temporal hint: 12.65 ms per
        // solve either way, profiles/r04_ab_hope_spmm_nt.jsonl; the block and its addends fit the chip's caches)
    }
}

// ------------------------------------------------------- Gram  P[slab] = X^T Y  (MFMA fp32)
// One wavefront per 32x32 output tile and row slab.  v_mfma_f32_32x32x2_f32 consumes two rows
// per issue: lane l supplies X[r + (l>>5)][ci + (l&31)] and Y[r + (l>>5)][cj + (l&31)] -- both
// coalesced 128-byte row segments.  Slab partials are summed in fp64 by hope_reduce_kernel
// (deterministic, no atomics).
__global__ __launch_bounds__(256) void hope_gram_kernel(int64_t n, const float *__restrict__ X, int ldx, int m1, const float *__restrict__ Y,
                                                        int ldy, int m2, int64_t rows_per_slab, int t2, int ntiles, float *__restrict__ P,
                                                        int m1p, int m2p)
{
    const int lane = lane_id();
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const int ti = tile / t2, tj = tile - ti * t2;
    const int ci = ti * 32 + (lane & 31), cj = tj * 32 + (lane & 31);
    const int h = lane >> 5;
    const int64_t r_begin = (int64_t)blockIdx.y * rows_per_slab;
    const int64_t r_end = r_begin + rows_per_slab < n ? r_begin + rows_per_slab : n;
    const bool vi = ci < m1, vj = cj < m2;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    int64_t r = r_begin;
    for (; r + 8 <= r_end; r += 8) {
        float a[4], bb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t rr = r + 2 * u + h;
            a[u] = vi ? X[rr * ldx + ci] : 0.f;
            bb[u] = vj ? Y[rr * ldy + cj] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bb[u], acc, 0, 0, 0);
    }
    for (; r < r_end; r += 2) {
        const int64_t rr = r + h;
        const float a = (vi && rr < r_end) ? X[rr * ldx + ci] : 0.f;
        const float bb = (vj && rr < r_end) ? Y[rr * ldy + cj] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, acc, 0, 0, 0);
    }
    float *Ps = P + (int64_t)blockIdx.y * m1p * m2p;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int row = ti * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;       // C/D map of the 32x32 MFMA
        Ps[(int64_t)row * m2p + tj * 32 + (lane & 31)] = acc[q];
    }
}

// Deterministic two-pass fp64 reduction of the slab partials (coalesced over the output index):
// pass 1: part[c][idx] = sum of slabs k = c, c+C, c+2C, ...   pass 2: G[idx] = sum_c part[c][idx].
__global__ void hope_reduce1_kernel(const float *__restrict__ P, int nslabs, int64_t stride, int m1, int m2, int m2p, int C, double *__restrict__ part)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (idx >= m1 * m2) return;
    const int i = idx / m2, j = idx - i * m2;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;                  // four loads in flight (the loop is latency bound); fixed order: deterministic
    const float *p = P + (int64_t)i * m2p + j;
    int k = c;
    for (; k + 3 * C < nslabs; k += 4 * C) {
        s0 += (double)p[k * stride]; s1 += (double)p[(k + C) * stride]; s2 += (double)p[(k + 2 * C) * stride]; s3 += (double)p[(k + 3 * C) * stride];
    }
    for (; k < nslabs; k += C) s0 += (double)p[k * stride];
    part[(int64_t)c * m1 * m2 + idx] = (s0 + s1) + (s2 + s3);
}
__global__ void hope_reduce2_kernel(const double *__restrict__ part, int C, int total, double *__restrict__ G, float *__restrict__ Gf)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int c = 0;
    for (; c + 8 <= C; c += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += part[(int64_t)(c + u) * total + idx];
    }
    for (; c < C; ++c) a[0] += part[(int64_t)c * total + idx];
    const double s = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    G[idx] = s;
    if (Gf) Gf[idx] = (float)s;                          // the rounding tsgemm() applies to host coefficients
}

// ------------------------------------------- tall-skinny GEMM  O = Src + alpha X C  (MFMA fp32)
// One wavefront per 32-row x 32-column output tile.  The MFMA's k pairs are re-labelled so that lane
// half h covers k0+4h..k0+4h+3 over four issues: every lane reads 16 contiguous bytes of its X row.
__global__ __launch_bounds__(256) void hope_tsgemm_kernel(int64_t n, const float *__restrict__ X, int ldx, int m, const float *__restrict__ Cm,
                                                          int ldc, int b2, float alpha, const float *Src, int lds_,
                                                          float *Out, int ldo, int ct_count)
{
    const int lane = lane_id();
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t rt = tile / ct_count;
    const int ct = (int)(tile - rt * ct_count);
    if (rt * 32 >= n) return;
    const int64_t irow = rt * 32 + (lane & 31);
    const int jcol = ct * 32 + (lane & 31);
    const int h = lane >> 5;
    const bool vr = irow < n, vc = jcol < b2;
    const float *px = X + irow * ldx;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    for (int k0 = 0; k0 < m; k0 += 8) {
        float a[4], bb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + 4 * h + t;
            a[t] = (vr && k < m) ? px[k] : 0.f;
            bb[t] = (vc && k < m) ? Cm[(int64_t)k * ldc + jcol] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], bb[t], acc, 0, 0, 0);
    }
    if (!vc) return;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t row = rt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (row < n) {
            const float s = Src ? Src[row * lds_ + jcol] : 0.f;
            Out[row * ldo + jcol] = s + alpha * acc[q];
        }
    }
}

// (Measured and dropped, round 4: the same product with a wavefront owning a 32-row block for ALL column tiles and the X tile staged through LDS with
// coalesced row reads -- bit-identical, X read once instead of once per column tile: 11.87 against 11.61 ms per symmetric solve, 100.0 against 101.1 ms
// per directed solve, profiles/r04_ab_hope_tsgemm_lds_dropped.jsonl.  The 16-byte-per-lane row reads above already hit the L1 lines the previous k steps
// brought in, and the LDS kernels' registers and 35-70 KB of LDS per block cost the occupancy the short k loops need.)
// ------------------------------------------- Ritz rotation + residual norms in one pass  (MFMA fp32)
// Out = V C (the Ritz vectors) and, without ever storing it, R = B C - (V C) diag(theta): only the column norms of R are wanted, so every 32 x 32
// tile leaves its columns' sums of squares in part[row tile][column] (fp32; summed in fp64, in a fixed order, by hope_colsum_kernel).  Same tiling
// and k relabelling as hope_tsgemm_kernel; V and B rows are read once per column tile.  Replaces three tall-skinny GEMMs and a full m x m Gram of R.
__global__ __launch_bounds__(256) void hope_ritz_kernel(int64_t n, const float *__restrict__ V, int ldv, const float *__restrict__ B, int ldb, int m,
                                                        const float *__restrict__ Cm, int ldc, int b2, const float *__restrict__ theta,
                                                        float *__restrict__ Out, int ldo, float *__restrict__ part, int b2p, int ct_count)
{
    const int lane = lane_id();
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t rt = tile / ct_count;
    const int ct = (int)(tile - rt * ct_count);
    if (rt * 32 >= n) return;
    const int64_t irow = rt * 32 + (lane & 31);
    const int jcol = ct * 32 + (lane & 31);
    const int h = lane >> 5;
    const bool vr = irow < n, vc = jcol < b2;
    const float *pv = V + irow * ldv, *pb = B + irow * ldb;
    f32x16 av, ab;
#pragma unroll
    for (int q = 0; q < 16; ++q) { av[q] = 0.f; ab[q] = 0.f; }
    for (int k0 = 0; k0 < m; k0 += 8) {
        float a[4], a2[4], bb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + 4 * h + t;
            const bool vk = k < m;
            a[t] = (vr && vk) ? pv[k] : 0.f;
            a2[t] = (vr && vk) ? pb[k] : 0.f;
            bb[t] = (vc && vk) ? Cm[(int64_t)k * ldc + jcol] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            av = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], bb[t], av, 0, 0, 0);
            ab = __builtin_amdgcn_mfma_f32_32x32x2f32(a2[t], bb[t], ab, 0, 0, 0);
        }
    }
    const float th = vc ? theta[jcol] : 0.f;
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t row = rt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        const float r = fmaf(-th, av[q], ab[q]);
        ss = fmaf(r, r, ss);                                  // (rows beyond n contribute exact zeros: their a, a2 were 0)
        if (vc && row < n) Out[row * ldo + jcol] = av[q];
    }
    ss += __shfl_xor(ss, 32);
    if (h == 0 && vc) part[rt * b2p + jcol] = ss;
}
// out[j] = sum over the row tiles of part[.][j], fp64, fixed order (one block per column)
__global__ __launch_bounds__(256) void hope_colsum_kernel(const float *__restrict__ part, int64_t ntr, int b2p, double *__restrict__ out)
{
    __shared__ double sh[256];
    const int j = blockIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t t = threadIdx.x;
    for (; t + 768 < ntr; t += 1024) {
        a0 += (double)part[t * b2p + j]; a1 += (double)part[(t + 256) * b2p + j]; a2 += (double)part[(t + 512) * b2p + j]; a3 += (double)part[(t + 768) * b2p + j];
    }
    for (; t < ntr; t += 256) a0 += (double)part[t * b2p + j];
    sh[threadIdx.x] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sh[threadIdx.x] += sh[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[j] = sh[0];
}

// Out[:, :b] = a X + b2 Y + c Z   (row-major blocks with their own leading dimensions)
__global__ void hope_lincomb_kernel(int64_t n, int b, float a, const float *X, int ldx, float b2, const float *Y, int ldy, float c, const float *Z,
                                    int ldz, float *Out, int ldo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * b) return;
    const int64_t i = t / b; const int j = (int)(t - i * b);
    Out[i * ldo + j] = a * X[i * ldx + j] + b2 * Y[i * ldy + j] + c * Z[i * ldz + j];
}

__global__ void hope_randn_kernel(float *X, int64_t n, int b, int ld, uint64_t seed)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = n * b;
    if (t * 4 >= total) return;
    const u32x4 r = philox4x32_10(seed, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), 0x686Fu /* 'ho' */, 0u);
    const float u1 = 1.0f - u01(r.x), u2 = u01(r.y), u3 = 1.0f - u01(r.z), u4 = u01(r.w);
    const float ra = sqrtf(-2.0f * logf(u1)), rb = sqrtf(-2.0f * logf(u3));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u2, &s0, &c0);
    sincosf(6.28318530717958647692f * u4, &s1, &c1);
    const float z[4] = {ra * c0, ra * s0, rb * c1, rb * s1};
    for (int k = 0; k < 4; ++k) {
        const int64_t e = t * 4 + k;
        if (e < total) X[(e / b) * ld + (e % b)] = z[k];
    }
}

// val[j] = the entry of column j with the largest magnitude (the first such row on ties): the sign convention of the outputs is
// "that entry of the left vector is positive".  One block per column; the block's rows are L2 / Infinity Cache hits.
__global__ __launch_bounds__(256) void hope_colmax_kernel(int64_t n, const float *__restrict__ X, int ld, float *__restrict__ val)
{
    __shared__ float s_abs[256], s_val[256];
    __shared__ long long s_idx[256];
    const int j = blockIdx.x;
    float best = -1.f, bv = 0.f; long long bi = 0;
    int64_t i = threadIdx.x;
    for (; i + 768 < n; i += 1024) {                              // four loads in flight; candidates are examined in ascending row order
        const float v0 = X[i * ld + j], v1 = X[(i + 256) * ld + j], v2 = X[(i + 512) * ld + j], v3 = X[(i + 768) * ld + j];
        if (fabsf(v0) > best) { best = fabsf(v0); bv = v0; bi = i; }
        if (fabsf(v1) > best) { best = fabsf(v1); bv = v1; bi = i + 256; }
        if (fabsf(v2) > best) { best = fabsf(v2); bv = v2; bi = i + 512; }
        if (fabsf(v3) > best) { best = fabsf(v3); bv = v3; bi = i + 768; }
    }
    for (; i < n; i += 256) {
        const float v = X[i * ld + j], a = fabsf(v);
        if (a > best) { best = a; bv = v; bi = i; }
    }
    s_abs[threadIdx.x] = best; s_val[threadIdx.x] = bv; s_idx[threadIdx.x] = bi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const float a = s_abs[threadIdx.x + st];
            if (a > s_abs[threadIdx.x] || (a == s_abs[threadIdx.x] && s_idx[threadIdx.x + st] < s_idx[threadIdx.x])) {
                s_abs[threadIdx.x] = a; s_val[threadIdx.x] = s_val[threadIdx.x + st]; s_idx[threadIdx.x] = s_idx[threadIdx.x + st];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) val[j] = s_val[0];
}

// The same selection in two coalesced passes (the one-block-per-column kernel above reads a column with a stride of ld floats: every 4-byte load
// costs a sector, 120 us at 100k x 96): pass 1 -- blockIdx.x = row chunk, blockIdx.y = group of 64 columns; a wavefront reads 64 consecutive columns
// of one row (256 contiguous bytes), four rows in flight per block; (|v|, v, row) candidates per (chunk, column) -- pass 2 -- one thread block per
// column folds the chunks.  Same rule: the largest magnitude, the FIRST such row on ties.
__global__ __launch_bounds__(256) void hope_colmax1_kernel(int64_t n, const float *__restrict__ X, int ld, int mc, int64_t rows_per_chunk,
                                                           float *__restrict__ pabs, float *__restrict__ pval, long long *__restrict__ pidx)
{
    __shared__ float s_abs[256], s_val[256];
    __shared__ long long s_idx[256];
    const int c = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int j = blockIdx.y * 64 + c;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = r0 + rows_per_chunk < n ? r0 + rows_per_chunk : n;
    float best = -1.f, bv = 0.f; long long bi = 0;
    if (j < mc)
        for (int64_t i = r0 + ph; i < r1; i += 4) {
            const float v = X[i * ld + j], a = fabsf(v);
            if (a > best) { best = a; bv = v; bi = i; }
        }
    s_abs[threadIdx.x] = best; s_val[threadIdx.x] = bv; s_idx[threadIdx.x] = bi;
    __syncthreads();
    if (ph == 0 && j < mc) {
        for (int q = 1; q < 4; ++q) {
            const float a = s_abs[c + 64 * q];
            const long long ii = s_idx[c + 64 * q];
            if (a > best || (a == best && ii < bi)) { best = a; bv = s_val[c + 64 * q]; bi = ii; }
        }
        const int64_t o = (int64_t)blockIdx.x * mc + j;
        pabs[o] = best; pval[o] = bv; pidx[o] = bi;
    }
}
__global__ __launch_bounds__(256) void hope_colmax2_kernel(int nchunks, int mc, const float *__restrict__ pabs, const float *__restrict__ pval,
                                                           const long long *__restrict__ pidx, float *__restrict__ val)
{
    // one block per column: every thread folds the chunks t, t + 256, ... (ascending), then the block's candidates meet in LDS under the same rule --
    // larger magnitude, or equal magnitude and the smaller row.  (The first version walked a column's 512 chunk candidates on ONE thread: 135 us.)
    __shared__ float s_abs[256], s_val[256];
    __shared__ long long s_idx[256];
    const int j = blockIdx.x;
    float best = -1.f, bv = 0.f; long long bi = 0x7fffffffffffffffLL;
    for (int ch = threadIdx.x; ch < nchunks; ch += 256) {
        const float a = pabs[(int64_t)ch * mc + j];
        const long long ii = pidx[(int64_t)ch * mc + j];
        if (a > best || (a == best && ii < bi)) { best = a; bv = pval[(int64_t)ch * mc + j]; bi = ii; }
    }
    s_abs[threadIdx.x] = best; s_val[threadIdx.x] = bv; s_idx[threadIdx.x] = bi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const float a = s_abs[threadIdx.x + st];
            if (a > s_abs[threadIdx.x] || (a == s_abs[threadIdx.x] && s_idx[threadIdx.x + st] < s_idx[threadIdx.x])) {
                s_abs[threadIdx.x] = a; s_val[threadIdx.x] = s_val[threadIdx.x + st]; s_idx[threadIdx.x] = s_idx[threadIdx.x + st];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) val[j] = s_val[0];
}

// ---------------------------------------------------------------------- solver state
struct Hope {
    int64_t n = 0, nnz = 0;
    float beta = 0.f;
    int mode = 0;                                    // 0: S = Katz (HOPE); 1: S = I + D^-1/2 A D^-1/2 (Laplacian Eigenmaps);
                                                     // 2: S = c I - (I-P)^T (I-P), P = D^-1 A (LLE), c in `beta`
    DevBuf<int64_t> rp, rpT;
    DevBuf<int32_t> ci, ciT;
    DevBuf<float> va, vaT;
    DevBuf<float> P;                                 // Gram slab partials (colmax carves other types out of it: sized in bytes / 4)
    DevBuf<double> G;                                // device fp64 Gram
    DevBuf<double> G2;                               // a second one (gram2: two Gram matrices, one host round trip)
    DevBuf<double> Gpart;                            // reduction scratch
    DevBuf<float> Csmall;                            // device small matrix for tsgemm
    hipStream_t s = nullptr;
    double spmm_count = 0, spmm_cols = 0, spmm_ms = 0; bool time_spmm = false;   // statistics of a solve (reset_solve_stats)
    std::vector<hipEvent_t> sp_pool; size_t sp_used = 0;      // (start, stop) pairs around SpMM runs; read once at the end of a solve
    struct CoefSlot { PinnedBuf<float> h; DevBuf<float> d; hipEvent_t done = nullptr; };
    CoefSlot coef[8]; unsigned coef_next = 0;                // pinned staging ring for the small host matrices tsgemm() takes
    DevBuf<float> ws[7];                                     // eigen-path workspace, kept across solves
    DevBuf<float> d_cm;                                      // 512 floats: column arg-max signs of the output step
    // Kernel-variant overrides (the gemhip_test_hope_* hooks set them; -1 = unset: the environment variable, else the default, decides)
    int force_spmm16 = -1;                                   // GEMHIP_HOPE_SPMM16: 0 = one row per wavefront, 1 = 16 lanes per row up to 128 columns
    int force_spmm16_u = -1;                                 // GEMHIP_HOPE_SPMM16_U: gathers in flight per row and round (2, 4, 8)
    int force_colmax2 = -1;                                  // GEMHIP_HOPE_COLMAX2: 0 = one block per column, 1 = two coalesced passes
    int last_spmm_c = 0, last_spmm_u = 0;                    // the instantiation spmm() launched last: <CPL16, U>, or <CPL> with U = 0 (the hooks report it)
    int err = 0;
    ~Hope()          // the events; the buffers free themselves
    {
        for (hipEvent_t e : sp_pool) hipEventDestroy(e);
        for (CoefSlot &c : coef) if (c.done) hipEventDestroy(c.done);
    }
};

#define HOPE_TRY(h, x) do { if (!(h).err) { hipError_t _e = (x); if (_e != hipSuccess) { (h).err = fail(GEMHIP_E_HIP, "hope: %s: %s", #x, hipGetErrorString(_e)); } } } while (0)

void spmm(Hope &H, bool transpose, float alpha, const float *X, int ldx, const float *Wadd, int ldw, float *Y, int ldy, int b,
          float wa = 1.0f, const float *W2 = nullptr, int ldw2 = 0, float wb = 0.f)
{
    if (H.err) return;
    const int64_t blocks = (H.n + 3) / 4;
    const dim3 grid((unsigned)((blocks + NUM_XCD - 1) / NUM_XCD * NUM_XCD)), blk(256);
    const int64_t *rp = transpose ? H.rpT : H.rp; const int32_t *ci = transpose ? H.ciT : H.ci; const float *va = transpose ? H.vaT : H.va;
    static const int use16_env = getenv("GEMHIP_HOPE_SPMM16") ? atoi(getenv("GEMHIP_HOPE_SPMM16")) : 1;
    const int use16 = H.force_spmm16 >= 0 ? H.force_spmm16 : use16_env;
    if (use16 && b <= 128) {
        const int64_t blocks16 = (H.n + 15) / 16;
        const dim3 grid16((unsigned)((blocks16 + NUM_XCD - 1) / NUM_XCD * NUM_XCD));
        const int c16 = (b + 15) / 16;
#define SPMM16(C, U) do { H.last_spmm_c = C; H.last_spmm_u = U; hipLaunchKernelGGL((hope_spmm16_kernel<C, U>), grid16, blk, 0, H.s, H.n, rp, ci, va, alpha, X, ldx, Wadd, ldw, Y, ldy, b, wa, W2, ldw2, wb); } while (0)
        // gathers in flight per row and round (GEMHIP_HOPE_SPMM16_U overrides): with a row's (column, value) pairs already in the group's registers the
        // rounds are separated by arithmetic only, and the bound is registers: U x ceil(b / 16) values per lane -- 8 up to 48 columns, 4 up to 80, 2 beyond
        // (round 5: 4.21 -> 3.92 ms of SpMM per eigen-path solve at SBM 100k/1M against round 4's U = 4 with a per-round pair prefetch)
        static const int uenv = getenv("GEMHIP_HOPE_SPMM16_U") ? atoi(getenv("GEMHIP_HOPE_SPMM16_U")) : 0;
        const int uu = H.force_spmm16_u > 0 ? H.force_spmm16_u : uenv > 0 ? uenv : (c16 <= 3 ? 8 : 4);
#define SPMM16_BY_U(C) do { if (uu >= 8) SPMM16(C, 8); else if (uu >= 4) SPMM16(C, 4); else SPMM16(C, 2); } while (0)
        if (c16 <= 1) SPMM16_BY_U(1);
        else if (c16 <= 2) SPMM16_BY_U(2);
        else if (c16 <= 3) SPMM16_BY_U(3);
        else if (c16 <= 4) SPMM16_BY_U(4);
        else if (c16 <= 5) SPMM16_BY_U(5);
        else if (c16 <= 6) { if (uu >= 4) SPMM16(6, 4); else SPMM16(6, 2); }
        else SPMM16(8, 2);
#undef SPMM16_BY_U
#undef SPMM16
        H.spmm_count += 1; H.spmm_cols += b;
        return;
    }
    const int cpl = (b + 63) / 64;
#define SPMM(C) do { H.last_spmm_c = C; H.last_spmm_u = 0; hipLaunchKernelGGL((hope_spmm_kernel<C>), grid, blk, 0, H.s, H.n, rp, ci, va, alpha, X, ldx, Wadd, ldw, Y, ldy, b, wa, W2, ldw2, wb); } while (0)
    if (cpl <= 1) SPMM(1); else if (cpl <= 2) SPMM(2); else if (cpl <= 4) SPMM(4); else SPMM(8);
#undef SPMM
    H.spmm_count += 1; H.spmm_cols += b;
}

// G (host, fp64, m1 x m2 row-major) = X[:, :m1]^T Y[:, :m2]
// device part: H.G (fp64, m1 x m2 row-major) = X^T Y ; optionally the same values rounded to fp32 into Gf (device)
static void gram_launch(Hope &H, const float *X, int ldx, int m1, const float *Y, int ldy, int m2, float *Gf, bool second = false)
{
    if (H.err || m1 == 0 || m2 == 0) return;
    const int t1 = (m1 + 31) / 32, t2 = (m2 + 31) / 32, m1p = t1 * 32, m2p = t2 * 32;
    const int ntiles_ = t1 * t2;
    // aim at ~8192 wavefronts (256 CUs x 32) whatever the tile count: slab partials stay ~32 MB
    int64_t want_slabs = std::max<int64_t>(1, 8192 / ntiles_);
    int64_t rows_per_slab = std::max<int64_t>(64, (H.n + want_slabs - 1) / want_slabs);
    rows_per_slab = (rows_per_slab + 7) / 8 * 8;
    const int nslabs = (int)((H.n + rows_per_slab - 1) / rows_per_slab);
    const size_t need = (size_t)nslabs * m1p * m2p * sizeof(float);
    HOPE_TRY(H, H.P.reserve(need / sizeof(float)));
    DevBuf<double> &Gd = second ? H.G2 : H.G;
    HOPE_TRY(H, Gd.reserve((size_t)m1 * m2));
    if (H.err) return;
    const int ntiles = t1 * t2;
    hipLaunchKernelGGL(hope_gram_kernel, dim3((ntiles + 3) / 4, nslabs), dim3(256), 0, H.s, H.n, X, ldx, m1, Y, ldy, m2, rows_per_slab, t2, ntiles,
                       H.P, m1p, m2p);
    const int Cr = std::min(nslabs, 64);
    HOPE_TRY(H, H.Gpart.reserve((size_t)Cr * m1 * m2));
    if (H.err) return;
    hipLaunchKernelGGL(hope_reduce1_kernel, dim3((m1 * m2 + 255) / 256, Cr), dim3(256), 0, H.s, H.P, nslabs, (int64_t)m1p * m2p, m1, m2, m2p, Cr, H.Gpart);
    hipLaunchKernelGGL(hope_reduce2_kernel, dim3((m1 * m2 + 255) / 256), dim3(256), 0, H.s, H.Gpart, Cr, m1 * m2, Gd, Gf);
}

void gram(Hope &H, const float *X, int ldx, int m1, const float *Y, int ldy, int m2, std::vector<double> &Gh)
{
    Gh.assign((size_t)m1 * m2, 0.0);
    if (H.err || m1 == 0 || m2 == 0) return;
    gram_launch(H, X, ldx, m1, Y, ldy, m2, nullptr);
    if (H.err) return;
    HOPE_TRY(H, hipMemcpyAsync(Gh.data(), H.G, (size_t)m1 * m2 * sizeof(double), hipMemcpyDeviceToHost, H.s));
    HOPE_TRY(H, hipStreamSynchronize(H.s));
}

// Out = Src + alpha X C with the coefficients already on the device
static void tsgemm_launch(Hope &H, const float *X, int ldx, int m, const float *Cd, int b2, float alpha, const float *Src, int lds_, float *Out, int ldo)
{
    const int ct = (b2 + 31) / 32;
    const int64_t tiles = ((H.n + 31) / 32) * ct;
    hipLaunchKernelGGL(hope_tsgemm_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, H.s, H.n, X, ldx, m, Cd, b2, b2, alpha, Src, lds_, Out, ldo, ct);
}

// Two Gram matrices, ONE host round trip: Ga = Xa^T Ya, Gb = Xb^T Yb (the slab partials and the reduction scratch are reused in stream order; only
// the fp64 results need a buffer each)
void gram2(Hope &H, const float *Xa, int ldxa, int ma1, const float *Ya, int ldya, int ma2, std::vector<double> &Ga,
           const float *Xb, int ldxb, int mb1, const float *Yb, int ldyb, int mb2, std::vector<double> &Gb)
{
    Ga.assign((size_t)ma1 * ma2, 0.0); Gb.assign((size_t)mb1 * mb2, 0.0);
    if (H.err || ma1 == 0 || ma2 == 0 || mb1 == 0 || mb2 == 0) return;
    gram_launch(H, Xa, ldxa, ma1, Ya, ldya, ma2, nullptr, false);
    gram_launch(H, Xb, ldxb, mb1, Yb, ldyb, mb2, nullptr, true);
    if (H.err) return;
    HOPE_TRY(H, hipMemcpyAsync(Ga.data(), H.G, Ga.size() * sizeof(double), hipMemcpyDeviceToHost, H.s));
    HOPE_TRY(H, hipMemcpyAsync(Gb.data(), H.G2, Gb.size() * sizeof(double), hipMemcpyDeviceToHost, H.s));
    HOPE_TRY(H, hipStreamSynchronize(H.s));
}

// The small host matrices of tsgemm() / ritz_rotate() go through a ring of pinned host / device slot pairs: no host synchronisation between the
// upload and the launch.  The next slot, holding >= need floats on both sides, once the launch that last read it (eight calls ago) has finished.
static Hope::CoefSlot &coef_slot(Hope &H, size_t need)
{
    Hope::CoefSlot &slot = H.coef[H.coef_next++ % 8];
    if (slot.done) HOPE_TRY(H, hipEventSynchronize(slot.done));
    else HOPE_TRY(H, hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    const size_t cap = std::max<size_t>(need, 16384);
    HOPE_TRY(H, slot.h.reserve(cap));
    HOPE_TRY(H, slot.d.reserve(cap));
    return slot;
}

// Out[:, :b2] = (Src ? Src : 0) + alpha * X[:, :m] * C   (C host fp64 m x b2 row-major)
void tsgemm(Hope &H, const float *X, int ldx, int m, const std::vector<double> &Ch, int b2, float alpha, const float *Src, int lds_, float *Out, int ldo)
{
    if (H.err || b2 == 0) return;
    Hope::CoefSlot &slot = coef_slot(H, (size_t)std::max(m, 1) * b2);
    if (H.err) return;
    for (size_t i = 0; i < (size_t)m * b2; ++i) slot.h[i] = (float)Ch[i];
    HOPE_TRY(H, hipMemcpyAsync(slot.d, slot.h, (size_t)m * b2 * sizeof(float), hipMemcpyHostToDevice, H.s));
    tsgemm_launch(H, X, ldx, m, slot.d, b2, alpha, Src, lds_, Out, ldo);
    HOPE_TRY(H, hipEventRecord(slot.done, H.s));
}

// Out[:, :b2] = V[:, :m] C  and  res2[j] = || B[:, :m] C[:, j] - theta[j] Out[:, j] ||^2   (C host fp64 m x b2 row-major; one pass over V and B, one
// host round trip for the b2 norms).  The Rayleigh-Ritz step's rotation and residuals: hope_ritz_kernel + hope_colsum_kernel.
void ritz_rotate(Hope &H, const float *V, int ldv, const float *B, int ldb, int m, const std::vector<double> &Ch, const std::vector<double> &theta, int b2,
                 float *Out, int ldo, std::vector<double> &res2)
{
    res2.assign(b2, 0.0);
    if (H.err || b2 == 0 || m == 0) return;
    const size_t need = (size_t)m * b2 + b2;
    Hope::CoefSlot &slot = coef_slot(H, need);
    const int ct = (b2 + 31) / 32, b2p = ct * 32;
    const int64_t ntr = (H.n + 31) / 32;
    const size_t pneed = (size_t)ntr * b2p * sizeof(float);
    HOPE_TRY(H, H.P.reserve(pneed / sizeof(float)));
    HOPE_TRY(H, H.G.reserve(b2));
    if (H.err) return;
    for (size_t i = 0; i < (size_t)m * b2; ++i) slot.h[i] = (float)Ch[i];
    for (int j = 0; j < b2; ++j) slot.h[(size_t)m * b2 + j] = (float)theta[j];
    HOPE_TRY(H, hipMemcpyAsync(slot.d, slot.h, need * sizeof(float), hipMemcpyHostToDevice, H.s));
    const int64_t tiles = ntr * ct;
    hipLaunchKernelGGL(hope_ritz_kernel, dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, H.s, H.n, V, ldv, B, ldb, m, slot.d, b2, b2, slot.d + (size_t)m * b2, Out, ldo,
                       H.P, b2p, ct);
    HOPE_TRY(H, hipEventRecord(slot.done, H.s));
    hipLaunchKernelGGL(hope_colsum_kernel, dim3(b2), dim3(256), 0, H.s, H.P, ntr, b2p, H.G);
    HOPE_TRY(H, hipMemcpyAsync(res2.data(), H.G, (size_t)b2 * sizeof(double), hipMemcpyDeviceToHost, H.s));
    HOPE_TRY(H, hipStreamSynchronize(H.s));
}

// val[j] = the entry of column j of X (n x mc, ld) with the largest magnitude, the first such row on ties (hope_colmax1/2_kernel; scratch: H.P)
void colmax(Hope &H, const float *X, int ld, int mc, float *val)
{
    if (H.err || mc <= 0) return;
    static const int two_pass_env = getenv("GEMHIP_HOPE_COLMAX2") ? atoi(getenv("GEMHIP_HOPE_COLMAX2")) : 1;
    const int two_pass = H.force_colmax2 >= 0 ? H.force_colmax2 : two_pass_env;
    if (!two_pass) { hipLaunchKernelGGL(hope_colmax_kernel, dim3(mc), dim3(256), 0, H.s, H.n, X, ld, val); return; }
    const int nchunks = (int)std::min<int64_t>(512, (H.n + 63) / 64);
    const int64_t rows_per_chunk = (H.n + nchunks - 1) / nchunks;
    const size_t per = (size_t)nchunks * mc;
    const size_t need = per * (sizeof(float) * 2 + sizeof(long long)) + 64;
    HOPE_TRY(H, H.P.reserve((need + 3) / sizeof(float)));
    if (H.err) return;
    long long *pidx = reinterpret_cast<long long *>(H.P.get());                    // (8-byte aligned part first)
    float *pabs = reinterpret_cast<float *>(pidx + per), *pval = pabs + per;
    hipLaunchKernelGGL(hope_colmax1_kernel, dim3(nchunks, (mc + 63) / 64), dim3(256), 0, H.s, H.n, X, ld, mc, rows_per_chunk, pabs, pval, pidx);
    hipLaunchKernelGGL(hope_colmax2_kernel, dim3(mc), dim3(256), 0, H.s, nchunks, mc, pabs, pval, pidx, val);
}

// W[:, :cols] -= V[:, :m] (V[:, :m]^T W[:, :cols]) with the coefficients kept in HBM: Gram, fp64 slab reduction, fp32 rounding and
// the tall-skinny GEMM are four back-to-back launches, no host round trip (same arithmetic as gram() + tsgemm()).
void project_out(Hope &H, const float *V, int ldv, int m, float *W, int ldw, int cols)
{
    if (H.err || m == 0 || cols == 0) return;
    const size_t need = (size_t)m * cols;
    HOPE_TRY(H, H.Csmall.reserve(need));
    if (H.err) return;
    gram_launch(H, V, ldv, m, W, ldw, cols, H.Csmall);
    if (H.err) return;
    tsgemm_launch(H, V, ldv, m, H.Csmall, cols, -1.0f, W, ldw, W, ldw);
}

// Out[:, :b] = a X + b2 Y + c Z over the H.n rows (hope_lincomb_kernel; Out may be one of the operands: every element is read, then written, by one thread)
void lincomb(Hope &H, int b, float a, const float *X, int ldx, float b2, const float *Y, int ldy, float c, const float *Z, int ldz, float *Out, int ldo)
{
    if (H.err) return;
    hipLaunchKernelGGL(hope_lincomb_kernel, dim3((unsigned)((H.n * b + 255) / 256)), dim3(256), 0, H.s, H.n, b, a, X, ldx, b2, Y, ldy, c, Z, ldz, Out, ldo);
}

// X[:, :b] = standard normal draws, a function of (seed, row, column, b) alone (hope_randn_kernel: four values per thread)
void randn(Hope &H, float *X, int b, int ld, uint64_t seed)
{
    if (H.err) return;
    const int64_t threads = (H.n * (int64_t)b + 3) / 4;
    hipLaunchKernelGGL(hope_randn_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, H.s, X, H.n, b, ld, seed);
}

// The device half of orth() / orth_scaled(): per pass the Gram matrix of the block's columns comes in, host_pass(keep, G, C) turns it into the
// keep x nk coefficients, and Y <- Y C goes out through Tmp.  Returns the number of columns kept.
template <typename HostPass>
int orth_passes(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, int passes, HostPass host_pass)
{
    int keep = b;
    for (int pass = 0; pass < passes && keep > 0 && !H.err; ++pass) {
        std::vector<double> G, C;
        gram(H, Y, ld, keep, Y, ld, keep, G);
        if (H.err) return 0;
        const int nk = host_pass(keep, G, C);
        if (nk == 0) return 0;
        tsgemm(H, Y, ld, keep, C, nk, 1.0f, nullptr, 0, Tmp, ldt);
        HOPE_TRY(H, hipMemcpy2DAsync(Y, (size_t)ld * sizeof(float), Tmp, (size_t)ldt * sizeof(float), (size_t)nk * sizeof(float), H.n, hipMemcpyDeviceToDevice, H.s));
        keep = nk;
    }
    return keep;
}

// Orthonormalise the b columns of Y (n x b, ld) in place (Tmp = scratch).  Well-conditioned blocks take a
// CholeskyQR step (Y <- Y R^-1); otherwise the Gram eigen-decomposition Y <- Y W L^-1/2 drops directions whose
// relative energy is below `tol` or whose absolute energy is below `abs_floor` (rank revealing: orth_pass).  Two passes.
int orth(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, double tol, double abs_floor = 0.0, int passes = 2, bool *remixed = nullptr)
{
    return orth_passes(H, Y, ld, b, Tmp, ldt, passes, [&](int keep, std::vector<double> &G, std::vector<double> &C) {
        const int nk = orth_pass(keep, G, tol, abs_floor, C, remixed);
        tol = 1e-12; abs_floor = 0.0;                          // second pass only polishes
        return nk;
    });
}

// Z = S X  (X: n x b):  W0 = beta A X ; Z <- W0 + beta A Z, `terms` times  => sum_{t=1..terms+1} (beta A)^t X.
// W0, T0, T1: scratch n x b with leading dimension ldt.
struct SpmmTimer {           // HIP events around a run of back-to-back SpMM launches (nothing else is enqueued in between)
    Hope &H;
    size_t idx = (size_t)-1;
    explicit SpmmTimer(Hope &h) : H(h)
    {
        if (!H.time_spmm || H.err) return;
        while (H.sp_pool.size() < H.sp_used + 2) { hipEvent_t e = nullptr; if (hipEventCreate(&e) != hipSuccess) return; H.sp_pool.push_back(e); }
        idx = H.sp_used; H.sp_used += 2;
        hipEventRecord(H.sp_pool[idx], H.s);
    }
    ~SpmmTimer() { if (idx != (size_t)-1) hipEventRecord(H.sp_pool[idx + 1], H.s); }       // no host wait here: spmm_time_collect() reads the pairs
};
// after the stream has been synchronised: total time between the recorded (start, stop) pairs
void spmm_time_collect(Hope &H)
{
    for (size_t i = 0; i + 1 < H.sp_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, H.sp_pool[i], H.sp_pool[i + 1]) == hipSuccess) H.spmm_ms += ms;
    }
    H.sp_used = 0;
}

// The two events around a solve (device window, stats[0]); owns them the way Buf owns memory.  create() also arms the SpMM timers.
struct SolveEvents {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    SolveEvents() = default;
    SolveEvents(const SolveEvents &) = delete;
    SolveEvents &operator=(const SolveEvents &) = delete;
    ~SolveEvents() { if (ev0) hipEventDestroy(ev0); if (ev1) hipEventDestroy(ev1); }
    int create(Hope &H, bool time_spmm)
    {
        if (!H.err) { HOPE_TRY(H, hipEventCreate(&ev0)); HOPE_TRY(H, hipEventCreate(&ev1)); H.time_spmm = time_spmm; }
        return H.err;
    }
};

void apply_S(Hope &H, const float *X, int ldx, int b, int terms, float *T0, float *T1, float *W0, int ldt, float *Out, int ldo)
{
    SpmmTimer timer(H);
    if (H.mode == 1) { spmm(H, false, 1.0f, X, ldx, X, ldx, Out, ldo, b); return; }          // (I + M) X
    if (H.mode == 2) {                                                                         // c X - N^T N X,  N = I - P
        spmm(H, false, -1.0f, X, ldx, X, ldx, W0, ldt, b);                                     // W0 = N X = X - P X
        spmm(H, true, 1.0f, W0, ldt, nullptr, 0, T0, ldt, b);                                  // T0 = P^T W0
        lincomb(H, b, H.beta, X, ldx, -1.0f, W0, ldt, 1.0f, T0, ldt, Out, ldo);                 // c X - W0 + P^T W0
        return;
    }
    spmm(H, false, H.beta, X, ldx, nullptr, 0, W0, ldt, b);
    if (terms == 0) {
        HOPE_TRY(H, hipMemcpy2DAsync(Out, (size_t)ldo * sizeof(float), W0, (size_t)ldt * sizeof(float), (size_t)b * sizeof(float), H.n, hipMemcpyDeviceToDevice, H.s));
        return;
    }
    const float *zin = W0;
    int ldin = ldt;
    for (int t = 0; t < terms; ++t) {
        const bool last = (t == terms - 1);
        float *zout = last ? Out : ((t & 1) ? T1 : T0);
        const int ldout = last ? ldo : ldt;
        spmm(H, false, H.beta, zin, ldin, W0, ldt, zout, ldout, b);
        zin = zout; ldin = ldout;
    }
}

// Z = S^T Y = beta A^T (I - beta A^T)^-1 Y :  R <- Y + beta A^T R, then Z = beta A^T R.
void apply_ST(Hope &H, const float *Y, int ldy, int b, int terms, float *T0, float *T1, int ldt, float *Out, int ldo)
{
    SpmmTimer timer(H);
    if (H.mode == 1) { spmm(H, false, 1.0f, Y, ldy, Y, ldy, Out, ldo, b); return; }          // symmetric operator
    if (H.mode == 2) {                                                                         // symmetric: same as apply_S (T0, T1 as scratch)
        spmm(H, false, -1.0f, Y, ldy, Y, ldy, T1, ldt, b);
        spmm(H, true, 1.0f, T1, ldt, nullptr, 0, T0, ldt, b);
        lincomb(H, b, H.beta, Y, ldy, -1.0f, T1, ldt, 1.0f, T0, ldt, Out, ldo);
        return;
    }
    const float *rin = Y; int ldr = ldy;
    for (int t = 0; t < terms; ++t) {
        float *rout = (t & 1) ? T1 : T0;
        spmm(H, true, H.beta, rin, ldr, Y, ldy, rout, ldt, b);
        rin = rout; ldr = ldt;
    }
    spmm(H, true, H.beta, rin, ldr, nullptr, 0, Out, ldo, b);
}

}  // namespace

// ------------------------------------------------------------------- host API
// Restarted block-Krylov SVD of the operator the Hope state encodes (H.mode).  out_mode 0: U sqrt(S), V sqrt(S) (HOPE);
// out_mode 1: unit right singular vectors only (symmetric operators: eigenvectors).  sigma ascending.
static int krylov_svd(Hope &H, int64_t n, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed,
                      int terms, double br, int out_mode, float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats)
{
    const int b = (int)std::min<int64_t>((int64_t)k + oversample, n);
    auto env_int = [](const char *name, int &v) -> const int * { const char *e = getenv(name); if (!e) return nullptr; v = atoi(e); return &v; };
    int basis_env = 0, depth_env = 0;
    const int mmax = krylov_basis_capacity(b, krylov_steps, n, env_int("GEMHIP_HOPE_BASIS_COLS", basis_env));
    GEMHIP_REQUIRE(b <= 512 && k <= mmax, "hope: k + oversample = %d too large (max 512)", b);
    const int ldm = (mmax + 31) / 32 * 32, ldb = (b + 31) / 32 * 32;
    DevBuf<float> Vall, Ball, T0, T1, W0, Tmp;
    auto dalloc = [&](DevBuf<float> &p, size_t cols) { HOPE_TRY(H, p.reserve((size_t)n * cols)); HOPE_TRY(H, hipMemset(p, 0, (size_t)n * cols * sizeof(float))); };
    dalloc(Vall, ldm); dalloc(Ball, ldm); dalloc(T0, ldb); dalloc(T1, ldb); dalloc(W0, ldb); dalloc(Tmp, ldm);
    SolveEvents tm;                 // (declared after the buffers: destroyed before they are freed, on every way out)
    if (tm.create(H, stats != nullptr)) return H.err;
    hipEventRecord(tm.ev0, H.s);

    randn(H, Vall, b, ldm, seed);
    int m0 = orth(H, Vall, ldm, b, Tmp, ldm, 1e-10);

    // Locking (deflation): a leading Ritz pair of the restart block whose residual ||S^T S v - sigma^2 v|| / sigma^2 fell
    // below lock_tol is frozen -- columns [0, nl) of Vall / Ball hold the locked right vectors and S v.  Later cycles only
    // orthogonalise against them: the Krylov blocks, the S applications and the projected eigenproblem shrink with every
    // lock.
    std::vector<double> sig_old(k, 0.0), sig(k, 0.0), Wv, ev, Zt, lock_sig, act_sig;   // ev: Ritz values DESCENDING, Zt: their vectors (column-major ma x mt)
    int mt = 0;
    int mc = 0, restarts_done = 0, nl = 0, ma = 0;
    bool v0_is_ritz = false;
    const bool locking = getenv("GEMHIP_HOPE_NO_LOCK") == nullptr;
    const double lock_tol = lock_tolerance(tol);
    const int b_min = krylov_b_min(b, oversample);
    double last_change = 1.0, last_residual = 1.0;
    bool exact = false;
    const bool debug = getenv("GEMHIP_HOPE_DEBUG") != nullptr;
    for (int rs = 0; rs <= max_restarts && !H.err; ++rs) {
        mc = nl + m0;
        int prev_off = nl, prev_b = m0, b_valid = nl;               // Ball columns [0, b_valid) hold S Vall
        const int steps = getenv("GEMHIP_HOPE_FIXED_DEPTH") ? krylov_steps : krylov_steps_after_lock(krylov_steps, mmax, nl, m0, env_int("GEMHIP_HOPE_DEPTH_COLS", depth_env));
        for (int j = 1; j <= steps && mc < mmax && !H.err; ++j) {
            // W = S^T S V_{j-1};  S V_{j-1} is also the block of B = S Vall the Rayleigh-Ritz step needs: keep it in place
            apply_S(H, Vall + prev_off, ldm, prev_b, terms, T0, T1, W0, ldb, Ball + prev_off, ldm);
            apply_ST(H, Ball + prev_off, ldm, prev_b, terms, T0, T1, ldb, W0, ldb);
            b_valid = prev_off + prev_b;
            // energy scale of the new block before projection (what is left after projecting out the basis is only kept if
            // it stands above fp32 rounding noise relative to this): the block is S^T S applied to orthonormal columns, so
            // sigma_1^4 from the previous cycle bounds it; the first cycle measures it
            double ref_energy = 0.0;
            if (rs > 0 && sig_old[0] > 0) ref_energy = sig_old[0] * sig_old[0] * sig_old[0] * sig_old[0];
            else {
                std::vector<double> D;
                gram(H, W0, ldb, prev_b, W0, ldb, prev_b, D);
                for (int c = 0; c < prev_b && !H.err; ++c) ref_energy = std::max(ref_energy, D[(size_t)c * prev_b + c]);
            }
            // full re-orthogonalisation against the basis so far, normalise, then project again on the normalised block:
            // a direction that survives the rank filter with small amplitude carries rounding noise that lies INSIDE
            // span(Vall); after normalisation that noise is O(eps / amplitude)
            float *Wp = W0;                                         // the part of the new block that is kept
            int wcols = prev_b;
            static const bool host_project = getenv("GEMHIP_HOPE_HOST_PROJECT") != nullptr;
            auto project = [&](int cols) {
                if (!host_project) { project_out(H, Vall, ldm, mc, Wp, ldb, cols); return; }
                std::vector<double> C;
                gram(H, Vall, ldm, mc, Wp, ldb, cols, C);
                tsgemm(H, Vall, ldm, mc, C, cols, -1.0f, Wp, ldb, Wp, ldb);
            };
            project(wcols);
            if (j == 1 && rs > 0 && sig_old[0] > 0) {
                // V_0 holds Ritz vectors of the previous cycle (descending sigma): what is left of S^T S v_c after
                // projecting out span(V_0) is exactly the residual  ||S^T S v_c - sigma_c^2 v_c||  of Ritz pair c
                std::vector<double> D;
                gram(H, W0, ldb, prev_b, W0, ldb, prev_b, D);
                double r2 = 0.0;
                const int want = k - nl;                            // wanted pairs still active (the leading ones of V_0)
                for (int c = 0; c < std::min(want, prev_b) && !H.err; ++c) r2 = std::max(r2, D[(size_t)c * prev_b + c]);
                last_residual = std::sqrt(r2) / (sig_old[0] * sig_old[0]);
                const int newl = locking && v0_is_ritz && !H.err ? krylov_lock_count(want, prev_b, b_min, act_sig, D, lock_tol) : 0;
                if (newl > 0) {
                    // columns [nl, nl+newl) of Vall / Ball already are v_c and S v_c: freezing them is a change of bookkeeping
                    for (int c = 0; c < newl; ++c) lock_sig.push_back(act_sig[c]);
                    nl += newl; Wp = W0 + newl; wcols = prev_b - newl;
                    if (debug) fprintf(stderr, "[hope] cycle %d locked %d pairs (%d in total)\n", rs, newl, nl);
                }
            }
            int nb = orth(H, Wp, ldb, wcols, Tmp, ldm, 1e-11, 1e-12 * ref_energy);
            if (nb > 0) {
                project(nb);
                nb = orth(H, Wp, ldb, nb, Tmp, ldm, 1e-9, 0.25, 1);   // unit columns: drop what lost half its norm; one polishing pass
            }
            nb = std::min(nb, mmax - mc);
            if (nb <= 0) break;
            HOPE_TRY(H, hipMemcpy2DAsync(Vall + mc, (size_t)ldm * sizeof(float), Wp, (size_t)ldb * sizeof(float), (size_t)nb * sizeof(float), n, hipMemcpyDeviceToDevice, H.s));
            prev_off = mc; prev_b = nb; mc += nb;
        }
        // B = S Vall for the blocks the Krylov steps did not produce (the last one)
        for (int off = b_valid; off < mc && !H.err; off += b) {
            const int bb = std::min(b, mc - off);
            apply_S(H, Vall + off, ldm, bb, terms, T0, T1, W0, ldb, Ball + off, ldm);
        }
        // Rayleigh-Ritz on the active columns: B_a^T B_a = Wv diag(ev) Wv^T
        ma = mc - nl;
        gram(H, Ball + nl, ldm, ma, Ball + nl, ldm, ma, Wv);
        if (H.err) break;
        mt = std::min(ma, b);                                       // restart block and output never use more than b Ritz pairs
        sym_eig_top(ma, Wv, mt, ev, Zt);
        GEMHIP_REQUIRE(mc >= k, "hope: Krylov space collapsed to %d < k=%d columns (rank-deficient S?)", mc, k);
        std::vector<double> all(lock_sig);
        for (int j = 0; j < std::min(mt, k); ++j) all.push_back(std::sqrt(std::max(ev[j], 0.0)));
        last_change = wanted_values(all, k, sig, sig_old);                                          // sig descending
        restarts_done = rs;
        if (debug) fprintf(stderr, "[hope] cycle %d basis %d (%d locked) sigma_k %.6g sigma_1 %.6g change %.3e residual(prev cycle) %.3e\n", rs, mc, nl, sig[k - 1], sig[0], last_change, last_residual);
        exact = (mc >= n);
        const bool done = exact || (rs > 0 && last_change < tol) || rs == max_restarts;
        if (done) break;
        // restart from the best right Ritz vectors of the active part:  V0 <- Vall[:, nl:] Wv[:, top]
        std::vector<double> C;
        const int nb = krylov_restart_block(mt, b, nl, b_min, ma, Zt, C);
        tsgemm(H, Vall + nl, ldm, ma, C, nb, 1.0f, nullptr, 0, Tmp, ldm);
        HOPE_TRY(H, hipMemcpy2DAsync(Vall + nl, (size_t)ldm * sizeof(float), Tmp, (size_t)ldm * sizeof(float), (size_t)nb * sizeof(float), n, hipMemcpyDeviceToDevice, H.s));
        bool remixed = false;
        m0 = orth(H, Vall + nl, ldm, nb, Tmp, ldm, 1e-10, 0.0, 2, &remixed);
        act_sig.assign(nb, 0.0);
        for (int j = 0; j < nb; ++j) act_sig[j] = std::sqrt(std::max(ev[j], 0.0));
        v0_is_ritz = !remixed && m0 == nb;
    }
    if (!H.err) {
        // U sqrt(S) = B W S^-1/2 ,  V sqrt(S) = Vall W S^1/2 over the locked columns (W = identity there) and the active Ritz
        // vectors; the k largest sigma, columns in ASCENDING sigma (svds order, hope.py:33)
        std::vector<OutCand> cand;
        for (int l = 0; l < nl; ++l) cand.push_back({lock_sig[l], 1.0, l});
        for (int j = 0; j < std::min(mt, k); ++j) cand.push_back({std::sqrt(std::max(ev[j], 0.0)), 1.0, nl + j});
        std::vector<double> Cu, Cv;
        select_outputs(cand, k, nl, ma, &Zt, true, out_mode == 1, sigma, Cu, Cv);
        // deterministic sign: largest-magnitude entry of each left vector positive (svds signs are arbitrary; the first such row on ties).  The
        // arg-maxima are taken on the device from the compact [n][k] product, the signs go into the coefficients and the product is formed again
        // (one more 36 us GEMM; rounds 1-2 flipped the n x k outputs in two host passes -- ~10 ms at 100k x 64, and impossible for device outputs)
        HOPE_TRY(H, H.d_cm.reserve(512));       // kept in the plan: no hipMalloc / hipFree (a device sync) per solve
        float *d_cm = H.d_cm;
        const std::vector<double> &Cref = U_sqrtS ? Cu : Cv;
        if (!H.err) tsgemm(H, U_sqrtS ? Ball : Vall, ldm, mc, Cref, k, 1.0f, nullptr, 0, Tmp, k);           // compact [n][k]
        std::vector<float> cm(k, 0.f);
        if (!H.err) {
            colmax(H, Tmp, k, k, d_cm);
            HOPE_TRY(H, hipMemcpyAsync(cm.data(), d_cm, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, H.s));
            HOPE_TRY(H, hipStreamSynchronize(H.s));
        }
        const bool any = flip_negative_columns(mc, k, std::vector<double>(cm.begin(), cm.end()), Cu, Cv);
        if (U_sqrtS) {
            if (any) tsgemm(H, Ball, ldm, mc, Cu, k, 1.0f, nullptr, 0, Tmp, k);
            HOPE_TRY(H, hipMemcpy(U_sqrtS, Tmp, (size_t)n * k * sizeof(float), hipMemcpyDefault /* host (gemhip_hope_plan_solve) or device (.._solve_device) destination */));
            tsgemm(H, Vall, ldm, mc, Cv, k, 1.0f, nullptr, 0, Tmp, k);
        } else if (any) tsgemm(H, Vall, ldm, mc, Cv, k, 1.0f, nullptr, 0, Tmp, k);
        HOPE_TRY(H, hipMemcpy(V_sqrtS, Tmp, (size_t)n * k * sizeof(float), hipMemcpyDefault /* host (gemhip_hope_plan_solve) or device (.._solve_device) destination */));
    }
    float ms = 0.f;
    if (!H.err) { hipEventRecord(tm.ev1, H.s); hipEventSynchronize(tm.ev1); hipEventElapsedTime(&ms, tm.ev0, tm.ev1); }
    if (!H.err) spmm_time_collect(H); else H.sp_used = 0;
    if (stats && !H.err) fill_solve_stats(stats, ms, H.spmm_count, H.spmm_cols, terms, mc, restarts_done, last_change, br, last_residual, H.spmm_ms);
    return H.err;
}


// ------------------------------------------------------------------ symmetric graphs: Chebyshev-filtered subspace iteration
// For A = A^T the Katz operator S = sum_t (beta A)^t = f(A), f(x) = beta x / (1 - beta x), has the eigenvectors of A: singular value
// |f(lambda)|, right vector q, left vector sign(f(lambda)) q.  The k largest |f(lambda)| sit at the two ends of A's spectrum, so the
// series is never applied: a block of k + oversample vectors is filtered with a Chebyshev polynomial of A that is bounded on the
// unwanted interval [-a_minus, a_plus] (|f| below a Ritz |f| taken from the middle of the oversampling columns) and grows outside it
// (one SpMM per degree, fused three-term recurrence), orthonormalised, and rotated by a (k + oversample)-sized Rayleigh-Ritz step on
// A.  Converged leading pairs are locked and projected out -- also INSIDE the filter, every few degrees -- so that the degree of a
// cycle is capped by the growth at the largest ACTIVE Ritz value rather than at the spectrum's edge (fp32: a direction known to ~1e-7
// relative must not be amplified past the wanted ones; 1e4 per cycle).  Against the block-Krylov path on S^T S this needs ~7x fewer
// SpMM columns, no n x 512 basis and no 512 x 512 projected eigenproblem (measured: DESIGN.md 3.2).
namespace {

// CholeskyQR on the column-NORMALISED Gram matrix, with the scaled Gram's eigen-decomposition as the fallback (orth_scaled_pass)
int orth_scaled(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, int passes)
{
    return orth_passes(H, Y, ld, b, Tmp, ldt, passes, [](int keep, std::vector<double> &G, std::vector<double> &C) { return orth_scaled_pass(keep, G, C); });
}

// Out = Op X for the eigen-path's operators: kind 0 / 1: Op = the CSR matrix (one SpMM); kind 2 (LLE): Op = N^T N, N = I - P, through the
// n x cols scratch T (two SpMMs).  alpha scales Op X; (wa, W) and (wb, W2) are the optional addends of the fused epilogue.
void apply_sym_op(Hope &H, int kind, float alpha, const float *X, int ldx, int cols, float *T, int ldt, float *Out, int ldo, float wa, const float *W,
                  int ldw, float wb, const float *W2, int ldw2)
{
    if (kind != 2) { spmm(H, false, alpha, X, ldx, W, ldw, Out, ldo, cols, wa, W2, ldw2, wb); return; }
    spmm(H, false, -1.0f, X, ldx, X, ldx, T, ldt, cols);                                        // T = X - P X
    if (!W && !W2) { spmm(H, true, -alpha, T, ldt, T, ldt, Out, ldo, cols, alpha); return; }     // alpha (T - P^T T)
    // alpha (T - P^T T) + wa W + wb W2: the SpMM epilogue takes two addends, so W and W2 are combined first (into Out, which the
    // epilogue then reads and overwrites element by element)
    lincomb(H, cols, W ? wa : 0.f, W ? W : T, W ? ldw : ldt, W2 ? wb : 0.f, W2 ? W2 : T, W2 ? ldw2 : ldt, 0.f, T, ldt, Out, ldo);
    spmm(H, true, -alpha, T, ldt, T, ldt, Out, ldo, cols, alpha, Out, ldo, 1.0f);
}

// V[:, :cols] <- T_m((Op - c I) / e) V[:, :cols]   (Chebyshev polynomial of the first kind; F[0..2]: n x cols scratch, leading dimension ldf;
// Ts: one more scratch block for kind 2).
// Q[:, :nl] (locked eigenvectors) is projected out of the two live terms of the recurrence every q degrees: what the locked directions
// regain through their residuals and through rounding grows by the filter's edge growth per degree, q keeps that below ~1e5.
void cheb_filter(Hope &H, int kind, float *V, int ldv, int cols, int m, double c, double e, float *const F[3], int ldf, float *Ts, const float *Q, int ldq,
                 int nl, int q)
{
    if (H.err || cols == 0 || m < 1) return;
    int i1 = 0, i0 = -1;                                                                                           // F[i1] = Y_j, F[i0] = Y_{j-1} (-1: V)
    { SpmmTimer timer(H); apply_sym_op(H, kind, (float)(1.0 / e), V, ldv, cols, Ts, ldf, F[0], ldf, (float)(-c / e), V, ldv, 0.f, nullptr, 0); }   // Y1 = (Op V - c V) / e
    int j = 2;
    while (j <= m && !H.err) {
        if (nl > 0 && q > 0 && (j - 1) % q == 0) {
            if (i0 < 0) project_out(H, Q, ldq, nl, V, ldv, cols); else project_out(H, Q, ldq, nl, F[i0], ldf, cols);
            project_out(H, Q, ldq, nl, F[i1], ldf, cols);
        }
        SpmmTimer timer(H);
        do {
            int i2 = 0;
            while (i2 == i1 || i2 == i0) ++i2;
            const float *y0 = i0 < 0 ? V : F[i0];
            apply_sym_op(H, kind, (float)(2.0 / e), F[i1], ldf, cols, Ts, ldf, F[i2], ldf, (float)(-2.0 * c / e), F[i1], ldf, -1.0f, y0, i0 < 0 ? ldv : ldf);   // Y_{j+1} = 2 (Op - c) Y_j / e - Y_{j-1}
            i0 = i1; i1 = i2; ++j;
        } while (j <= m && !(nl > 0 && q > 0 && (j - 1) % q == 0));
    }
    HOPE_TRY(H, hipMemcpy2DAsync(V, (size_t)ldv * sizeof(float), F[i1], (size_t)ldf * sizeof(float), (size_t)cols * sizeof(float), H.n, hipMemcpyDeviceToDevice, H.s));
}

}  // namespace

// Returns H.err; *fell_back = true when the iteration broke down or did not converge in max_cycles (the caller then runs the
// general block-Krylov solver); outputs are only written on success.
// kind 0: the Katz map f(x) = beta x / (1 - beta x) (HOPE; two-sided, outputs U sqrt(s), V sqrt(s));  kind 1: f(x) = 1 + x on the
// normalised adjacency D^-1/2 A D^-1/2, spectrum in [-1, 1] (Laplacian Eigenmaps: the largest eigenvalues of I + M; one-sided, outputs
// unit eigenvectors and f);  kind 2: f(x) = c - x on N^T N, N = I - P, spectrum in [0, c], c = H.beta (LLE: the SMALLEST eigenvalues;
// one-sided at the lower end, two SpMMs per application, outputs unit eigenvectors and f).
static int sym_filter_svd(Hope &H, int kind, int64_t n, int32_t k, int32_t oversample, int32_t max_cycles, float tol, uint64_t seed, double br,
                          float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats, bool *fell_back)
{
    *fell_back = false;
    const auto ht0 = std::chrono::steady_clock::now();       // host timeline of the call (printed under GEMHIP_HOPE_DEBUG)
    const double beta = H.beta;
    auto fk = [&](double x) { return sym_f(kind, beta, x); };
    const int b = (int)std::min<int64_t>((int64_t)k + oversample, n);
    // the SpMM kernels carry at most 512 block columns (CPL = 8) and the column-norm scratch below holds 512 floats: a wider block must be
    // refused here exactly as krylov_svd refuses it, not truncated silently
    GEMHIP_REQUIRE(b <= 512, "hope: k + oversample = %d too large (max 512)", b);
    const int ldv = (b + 31) / 32 * 32;
    const bool debug = getenv("GEMHIP_HOPE_DEBUG") != nullptr;
    double amp = 1e4, amp0 = 1e3;
    if (const char *e = getenv("GEMHIP_HOPE_SYM_AMP")) amp = std::max(10.0, atof(e));
    if (const char *e = getenv("GEMHIP_HOPE_SYM_AMP0")) amp0 = std::max(10.0, atof(e));
    const bool fused_rr = !(getenv("GEMHIP_HOPE_SYM_FUSED_RR") && atoi(getenv("GEMHIP_HOPE_SYM_FUSED_RR")) == 0);
    int max_degree = 32;                                    // measured at SBM 100k/1M: 30-32 per cycle is cheapest (scripts/ab_hope_sym.py)
    if (const char *e = getenv("GEMHIP_HOPE_SYM_MAXDEG")) max_degree = std::max(2, atoi(e));
    float *Vall = nullptr, *Bm = nullptr, *F[3] = {nullptr, nullptr, nullptr}, *Tmp = nullptr, *colv = nullptr;
    // workspace: seven n x ldv blocks kept in the solver state across solves (a plan is solved repeatedly; hipMalloc / hipFree of
    // ~40 MB blocks cost more than a filter cycle)
    auto walloc = [&](int slot, float **p, size_t elems) {
        if (elems > H.ws[slot].capacity() && !H.err) {
            HOPE_TRY(H, H.ws[slot].reserve(elems));
            // zeroed when allocated: the padding columns (b .. ldv) are never written and never read as data, but they must not hold NaN patterns for
            // the tools that scan whole buffers; a reused block holds the finite values of the previous solve (seven memsets per solve saved)
            HOPE_TRY(H, hipMemsetAsync(H.ws[slot], 0, elems * sizeof(float), H.s));
        }
        *p = H.ws[slot];
    };
    walloc(0, &Vall, (size_t)n * ldv); walloc(1, &Bm, (size_t)n * ldv); walloc(2, &F[0], (size_t)n * ldv); walloc(3, &F[1], (size_t)n * ldv);
    walloc(4, &F[2], (size_t)n * ldv); walloc(5, &Tmp, (size_t)n * ldv); walloc(6, &colv, 512);
    SolveEvents tm;
    if (tm.create(H, stats != nullptr)) return H.err;
    hipEventRecord(tm.ev0, H.s);
    const auto ht1 = std::chrono::steady_clock::now();

    randn(H, Vall, b, ldv, seed);
    int ma = orth_scaled(H, Vall, ldv, b, Tmp, ldv, 1), nl = 0;      // (one CholeskyQR pass: a Gaussian block is well conditioned, and the first filter is followed by the full CholeskyQR2)

    const SymSpectrum sp = sym_spectrum(kind, beta, br);
    const double L = sp.L, lock_tol = lock_tolerance(tol);
    double lo, hi, tau_prev = 0.0;
    sym_first_interval(kind, L, lo, hi);
    const int b_min = std::min(b, (int)oversample + 2);      // the active block keeps its oversampling columns
    std::vector<double> lock_lam, th, res, sig(k, 0.0), sig_old(k, 0.0);
    double last_change = 1.0, last_residual = 1.0;
    int cycles = 0;
    bool converged = false;
    for (int cyc = 0; cyc < max_cycles && !H.err; ++cyc) {
        cycles = cyc + 1;
        const SymCycle cy = sym_cycle_plan(lo, hi, sp.smin, sp.smax, th, nl, cyc, amp, amp0, max_degree);
        float *Va = Vall + nl;
        cheb_filter(H, kind, Va, ldv, ma, cy.m, cy.c, cy.e, F, ldv, Bm, Vall, ldv, nl, cy.q);
        // CholeskyQR2 + Rayleigh-Ritz on A over the active block.  With locked vectors the projection is repeated between the two passes (the first pass
        // rescales the block).  FUSED (default; GEMHIP_HOPE_SYM_FUSED_RR=0 for the A/B): the second CholeskyQR pass is not applied to the block -- after the
        // first pass Y1 is orthonormal to ~1e-3, so G2 = Y1^T Y1 and H1 = Y1^T (A Y1) are taken in ONE host round trip (gram2), C2 = chol(G2)^-1 and
        // the projected matrix (Y1 C2)^T A (Y1 C2) = C2^T H1 C2 are formed on the host in fp64, and the Ritz rotation below takes Y1 straight to the Ritz
        // vectors with the coefficients C2 W: one synchronisation, one Gram, one tall-skinny GEMM and one block copy less per cycle, and Q = Y1 C2 is
        // never rounded to fp32.  A Cholesky that loses a pivot (rank loss) falls back to the two-pass sequence.
        int keep;
        std::vector<double> Hh, ev, C2;                           // C2: empty = identity
        bool rr_have = false;
        if (fused_rr) {
            if (nl) project_out(H, Vall, ldv, nl, Va, ldv, ma);
            keep = orth_scaled(H, Va, ldv, ma, Tmp, ldv, 1);
            if (keep > 0 && nl) project_out(H, Vall, ldv, nl, Va, ldv, keep);
            if (H.err) break;
            if (nl + keep < k + 1 || keep < 2) { if (debug) fprintf(stderr, "[hope-sym] block collapsed to %d columns\n", keep); break; }
            { SpmmTimer timer(H); apply_sym_op(H, kind, 1.0f, Va, ldv, keep, F[0], ldv, Bm, ldv, 1.0f, nullptr, 0, 0.f, nullptr, 0); }
            std::vector<double> G2;
            gram2(H, Va, ldv, keep, Va, ldv, keep, G2, Va, ldv, keep, Bm, ldv, keep, Hh);
            if (H.err) break;
            if (rr_project(keep, G2, Hh, C2)) rr_have = true;
            else {
                keep = orth_scaled(H, Va, ldv, keep, Tmp, ldv, 1);      // (rank loss: the rank-revealing second pass, then the plain Rayleigh-Ritz step)
                if (H.err) break;
            }
        } else if (nl) {
            project_out(H, Vall, ldv, nl, Va, ldv, ma);
            keep = orth_scaled(H, Va, ldv, ma, Tmp, ldv, 1);
            if (keep > 0) { project_out(H, Vall, ldv, nl, Va, ldv, keep); keep = orth_scaled(H, Va, ldv, keep, Tmp, ldv, 1); }
        } else keep = orth_scaled(H, Va, ldv, ma, Tmp, ldv, 2);
        if (H.err) break;
        if (nl + keep < k + 1 || keep < 2) { if (debug) fprintf(stderr, "[hope-sym] block collapsed to %d columns\n", keep); break; }
        ma = keep;
        if (!rr_have) {
            { SpmmTimer timer(H); apply_sym_op(H, kind, 1.0f, Va, ldv, ma, F[0], ldv, Bm, ldv, 1.0f, nullptr, 0, 0.f, nullptr, 0); }
            gram(H, Va, ldv, ma, Bm, ldv, ma, Hh);
            if (H.err) break;
        }
        symmetrise(ma, Hh);
        sym_eig(ma, Hh, ev);                                                          // ascending; column j of Hh = eigenvector j
        std::vector<double> C, Ct;
        ritz_order(ma, Hh, ev, kind, beta, C2, th, C, Ct);
        // residuals R = B C - V C diag(theta), then the block becomes its Ritz vectors V C.  FUSED (default with the fused Rayleigh-Ritz step): one
        // pass computes V C and the column norms of R without storing R (ritz_rotate); otherwise three tall-skinny GEMMs and the Gram matrix of R
        res.assign(ma, 0.0);
        if (fused_rr) {
            std::vector<double> r2;
            ritz_rotate(H, Va, ldv, Bm, ldv, ma, C, th, ma, Tmp, ldv, r2);
            HOPE_TRY(H, hipMemcpy2DAsync(Va, (size_t)ldv * sizeof(float), Tmp, (size_t)ldv * sizeof(float), (size_t)ma * sizeof(float), n, hipMemcpyDeviceToDevice, H.s));
            if (H.err) break;
            for (int j = 0; j < ma; ++j) res[j] = std::sqrt(std::max(r2[j], 0.0));
        } else {
            tsgemm(H, Va, ldv, ma, Ct, ma, 1.0f, nullptr, 0, F[0], ldv);
            tsgemm(H, Bm, ldv, ma, C, ma, 1.0f, F[0], ldv, F[0], ldv);
            tsgemm(H, Va, ldv, ma, C, ma, 1.0f, nullptr, 0, Tmp, ldv);
            HOPE_TRY(H, hipMemcpy2DAsync(Va, (size_t)ldv * sizeof(float), Tmp, (size_t)ldv * sizeof(float), (size_t)ma * sizeof(float), n, hipMemcpyDeviceToDevice, H.s));
            std::vector<double> RR;
            gram(H, F[0], ldv, ma, F[0], ldv, ma, RR);
            if (H.err) break;
            for (int j = 0; j < ma; ++j) res[j] = std::sqrt(std::max(RR[(size_t)j * ma + j], 0.0));
        }
        // wanted values so far: the k largest |f| over the locked eigenvalues and the active Ritz values
        std::vector<double> all;
        for (double l : lock_lam) all.push_back(std::fabs(fk(l)));
        for (int j = 0; j < ma; ++j) all.push_back(std::fabs(fk(th[j])));
        last_change = wanted_values(all, k, sig, sig_old);
        const int want = k - nl;                                                       // wanted pairs still active: the leading ones
        const double rmax = last_residual = sym_residual_scale(want, th, res, L, sp.res_floor);
        if (debug)
            fprintf(stderr, "[hope-sym] cycle %d degree %d interval [%.4f, %.4f] locked %d active %d sigma_k %.6g sigma_1 %.6g change %.3e residual %.3e\n",
                    cyc, cy.m, lo, hi, nl, ma, sig[k - 1], sig[0], last_change, rmax);
        if (cyc > 0 && last_change < tol && rmax < 1e-2) { converged = true; break; }
        const int newl = sym_lock_count(want, b_min, th, res, lock_tol, sp.res_floor);
        if (newl > 0) {                                                                // leading columns of the active block: bookkeeping only
            for (int j = 0; j < newl; ++j) lock_lam.push_back(th[j]);
            th.erase(th.begin(), th.begin() + newl); res.erase(res.begin(), res.begin() + newl);
            nl += newl; ma -= newl;
        }
        sym_next_interval(kind, beta, L, k - nl, th, tau_prev, lo, hi);
    }
    if (!H.err && !converged) { *fell_back = true; return GEMHIP_OK; }
    const auto ht2 = std::chrono::steady_clock::now();
    if (!H.err) {
        std::vector<OutCand> cand;
        for (int l = 0; l < nl; ++l) cand.push_back({std::fabs(fk(lock_lam[l])), fk(lock_lam[l]) < 0 ? -1.0 : 1.0, l});      // u = sign(f(lambda)) q
        for (int j = 0; j < ma; ++j) cand.push_back({std::fabs(fk(th[j])), fk(th[j]) < 0 ? -1.0 : 1.0, nl + j});
        const int mc = nl + ma;
        // sign convention (largest-magnitude entry of each left vector positive) from the basis columns themselves
        colmax(H, Vall, ldv, mc, colv);
        std::vector<float> cm(mc, 0.f);
        HOPE_TRY(H, hipMemcpyAsync(cm.data(), colv, (size_t)mc * sizeof(float), hipMemcpyDeviceToHost, H.s));
        HOPE_TRY(H, hipStreamSynchronize(H.s));
        std::vector<double> Cu, Cv, umax(k, 0.0);
        select_outputs(cand, k, nl, ma, nullptr, false, kind >= 1, sigma, Cu, Cv);
        for (int r = 0; r < k; ++r) umax[k - 1 - r] = cand[r].sgn * cm[cand[r].col];
        flip_negative_columns(mc, k, umax, Cu, Cv);
        if (U_sqrtS) {
            tsgemm(H, Vall, ldv, mc, Cu, k, 1.0f, nullptr, 0, Tmp, k);
            HOPE_TRY(H, hipMemcpy(U_sqrtS, Tmp, (size_t)n * k * sizeof(float), hipMemcpyDefault /* host (gemhip_hope_plan_solve) or device (.._solve_device) destination */));
        }
        tsgemm(H, Vall, ldv, mc, Cv, k, 1.0f, nullptr, 0, Tmp, k);
        HOPE_TRY(H, hipMemcpy(V_sqrtS, Tmp, (size_t)n * k * sizeof(float), hipMemcpyDefault /* host (gemhip_hope_plan_solve) or device (.._solve_device) destination */));
        // (measured: forming both outputs first and copying them out from two host threads side by side is 0.3 ms SLOWER per solve)
    }
    float ms = 0.f;
    const auto ht3 = std::chrono::steady_clock::now();
    if (!H.err) { hipEventRecord(tm.ev1, H.s); hipEventSynchronize(tm.ev1); hipEventElapsedTime(&ms, tm.ev0, tm.ev1); }
    const auto ht4 = std::chrono::steady_clock::now();
    if (!H.err) spmm_time_collect(H); else H.sp_used = 0;
    if (debug) {
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b2) { return std::chrono::duration<double, std::micro>(b2 - a).count(); };
        fprintf(stderr, "[hope-sym] host timeline (us): set-up %.0f | cycles %.0f | outputs %.0f | final event %.0f | spmm timers %.0f ; device window %.0f\n",
                us(ht0, ht1), us(ht1, ht2), us(ht2, ht3), us(ht3, ht4), us(ht4, std::chrono::steady_clock::now()), ms * 1e3);
    }
    if (stats && !H.err)      // stats[3]: no Katz series, f on the eigenvalues (-1: the Laplacian-Eigenmaps map, -2: LLE)
        fill_solve_stats(stats, ms, H.spmm_count, H.spmm_cols, kind >= 1 ? -(double)kind : 0.0, nl + ma, cycles, last_change, br, last_residual, H.spmm_ms);
    return H.err;
}

// ------------------------------------------------------------------ setup steps the operator entry points share
namespace {

// The CSR checks of gemhip_hope_plan_create, gemhip_lap_eigmap and gemhip_lle; `who` is the entry point's message prefix.  Host reads only: it
// runs before the entry point's first HIP call, so a bad graph is GEMHIP_E_INVALID on a machine without a GPU too.
int check_csr(const char *who, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col)
{
    int64_t e = 0;
    const CsrError err = check_csr_arrays(n, nnz, row_ptr, col, &e);
    GEMHIP_REQUIRE(err != CsrError::BAD_ARGUMENTS, "%s: bad CSR arguments", who);
    GEMHIP_REQUIRE(err != CsrError::ROW_PTR, "%s: row_ptr inconsistent with nnz", who);
    GEMHIP_REQUIRE(err != CsrError::COLUMN, "%s: column %d outside [0,%lld)", who, col[e], (long long)n);
    return GEMHIP_OK;
}

// A (values va) and, if T is given, A^T into H; returns H.err.  `who` (an entry point's message prefix, or null): first see that there is a device at all.
int upload_csr(Hope &H, const char *who, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *va, const CsrT *T)
{
    int devid = 0;
    if (who && hipGetDevice(&devid) != hipSuccess) return H.err = fail(GEMHIP_E_HIP, "%s: no HIP device", who);
    H.n = n; H.nnz = nnz;
    HOPE_TRY(H, H.rp.upload(row_ptr, n + 1)); HOPE_TRY(H, H.ci.upload(col, nnz)); HOPE_TRY(H, H.va.upload(va, nnz));
    if (!T) return H.err;
    HOPE_TRY(H, H.rpT.upload(T->rp.data(), n + 1)); HOPE_TRY(H, H.ciT.upload(T->ci.data(), nnz)); HOPE_TRY(H, H.vaT.upload(T->va.data(), nnz));
    return H.err;
}

// ... with the caller's weights as they are (default 1): the building-block entry point and the test hooks
void upload_csr_w(Hope &H, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, bool with_transpose)
{
    std::vector<float> va(std::max<int64_t>(nnz, 1), 1.0f);
    if (w) std::copy(w, w + nnz, va.begin());
    CsrT T;
    if (with_transpose) T = transpose_csr(n, nnz, row_ptr, col, va.data());
    upload_csr(H, nullptr, n, nnz, row_ptr, col, va.data(), with_transpose ? &T : nullptr);
}

// Power iteration on a symmetric positive semi-definite operator with the one-column SpMM.  X2 = [x | z] is an n x 2 block, so that one Gram launch
// returns both norms; fill_z(X2, tmp) writes z = Op x into column 1 (tmp: n floats of scratch); x starts at 1 + a sin(f (i + 1)).  At most max_it steps;
// from step min_it on it stops when the estimate moved by <= rel_tol of itself -- the estimate is ||z|| / ||x||, with root_estimate its square root (Op = A^T A,
// the caller is after sigma_max(A)).  Returns ||z|| / ||x|| of the last step (0: none completed; from below: callers add a margin); errors are in H.err.
template <typename FillZ>
double power_iteration(Hope &H, double a, double f, int max_it, int min_it, double rel_tol, bool root_estimate, FillZ fill_z)
{
    std::vector<float> x0((size_t)H.n * 2, 0.f);
    for (int64_t i = 0; i < H.n; ++i) x0[(size_t)i * 2] = (float)(1.0 + a * std::sin(f * (double)(i + 1)));
    DevBuf<float> X2, tmp;
    HOPE_TRY(H, X2.upload(x0.data(), x0.size()));
    HOPE_TRY(H, tmp.reserve(H.n));
    double ratio = 0.0, est = 0.0;
    for (int it = 0; it < max_it && !H.err; ++it) {
        fill_z(X2.get(), tmp.get());
        std::vector<double> G2;
        gram(H, X2, 2, 2, X2, 2, 2, G2);
        if (H.err) break;
        const double nx = G2[0], nz = G2[3];
        if (!(nz > 0.0) || !(nx > 0.0) || !std::isfinite(nz)) break;
        const double prev = est;
        ratio = std::sqrt(nz / nx);
        est = root_estimate ? std::sqrt(ratio) : ratio;
        lincomb(H, 1, (float)(1.0 / std::sqrt(nz)), X2 + 1, 2, 0.f, X2 + 1, 2, 0.f, X2 + 1, 2, X2, 2);      // x = z / |z|
        if (it >= min_it && std::fabs(est - prev) <= rel_tol * est) break;
    }
    HOPE_TRY(H, hipStreamSynchronize(H.s));
    return ratio;
}

void reset_solve_stats(Hope &H) { H.err = 0; H.spmm_count = 0; H.spmm_cols = 0; H.spmm_ms = 0; H.sp_used = 0; reset_eig_stats(); }

// One solve of the operator H holds (H.mode), with fresh statistics.  Symmetric operators (`symmetric`: always for Laplacian Eigenmaps and LLE;
// HOPE passes A == A^T and beta > 0 -- undirected graphs: every GEM example and the SBM benchmark) take the Chebyshev-filtered eigen-path:
// GEMHIP_HOPE_SYM=0 disables it, =1 takes it at any size; by default graphs under 16384 nodes stay on the block-Krylov solver (already milliseconds
// there).  If the eigen-path does not converge: the general solver, statistics reset again.  terms, br, out_mode: see krylov_svd.
int solve_operator(Hope &H, bool symmetric, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed,
                   int terms, double br, int out_mode, float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats)
{
    reset_solve_stats(H);
    const char *sym_env = getenv("GEMHIP_HOPE_SYM");
    const bool sym_ok = symmetric && (int64_t)k + oversample + 1 < H.n;
    if (sym_ok && (sym_env ? atoi(sym_env) != 0 : (H.n >= 16384 && 8 * ((int64_t)k + oversample) <= H.n))) {
        bool fell_back = false;
        const int rc = sym_filter_svd(H, H.mode, H.n, k, oversample, std::max(40, 3 * (int)max_restarts), tol, seed, br, U_sqrtS, V_sqrtS, sigma, stats, &fell_back);
        if (rc || !fell_back) return rc;
        reset_solve_stats(H);
    }
    return krylov_svd(H, H.n, k, oversample, krylov_steps, max_restarts, tol, seed, terms, br, out_mode, U_sqrtS, V_sqrtS, sigma, stats);
}

}  // namespace

struct gemhip_hope_plan {
    Hope H;
    int terms = 1;
    double br = 0.0;
    bool symmetric = false;                          // A == A^T entry for entry (columns sorted within rows): the eigen-path applies
    double frob2_A = 0.0;                            // sum of the squared edge weights: ||beta A||_F^2 = beta^2 x this (gemhip_hope_plan_svd_error)
};

// Graph-dependent setup of the Katz operator: A and A^T in CSR on the device, number of series terms from sigma_max(A).
static int hope_setup(gemhip_hope_plan &P, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta)
{
    if (const int rc = check_csr("hope", n, nnz, row_ptr, col)) return rc;
    Hope &H = P.H;
    H.beta = beta;
    std::vector<float> va(std::max<int64_t>(nnz, 1));                    // values default to 1
    for (int64_t e = 0; e < nnz; ++e) { va[e] = w ? w[e] : 1.0f; P.frob2_A += (double)va[e] * (double)va[e]; }
    const CsrT T = transpose_csr(n, nnz, row_ptr, col, va.data());
    P.symmetric = csr_is_symmetric(n, nnz, row_ptr, T);
    if (upload_csr(H, "hope", n, nnz, row_ptr, col, va.data(), &T)) return H.err;
    // sigma_max(A) >= rho(A) by power iteration on A^T A (at most 40 steps; the 10 % margin covers what the stopping rule leaves)
    double rho = std::sqrt(power_iteration(H, 0.37, 12.9898, 40, 4, 1e-3, true, [&](float *X2, float *y) {
        spmm(H, false, 1.0f, X2, 2, nullptr, 0, y, 1, 1);                            // y = A x
        spmm(H, true, 1.0f, y, 1, nullptr, 0, X2 + 1, 2, 1);                         // z = A^T y
    }));
    if (H.err) return H.err;
    rho = std::min(std::max(rho * 1.1, 1e-30), abs_sum_bound(n, row_ptr, col, va.data()));     // the max absolute row / column sums bound it too
    const double br = std::fabs((double)beta) * rho;
    if (!(br < 0.95))
        return fail(GEMHIP_E_NOTCONVERGED, "hope: beta*rho(A) ~ %.3f >= 0.95: the Katz series (I - beta A)^-1 = sum (beta A)^t does not converge fast "
                                           "enough on this graph (the reference forms the dense inverse); lower beta", br);
    P.terms = katz_terms(br); P.br = br;
    return GEMHIP_OK;
}

extern "C" int gemhip_hope_plan_create(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta,
                                       gemhip_hope_plan_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "hope_plan_create: out is NULL");
    *out = nullptr;
    auto *P = new gemhip_hope_plan();
    const int rc = hope_setup(*P, n, nnz, row_ptr, col, w, beta);
    if (rc) { delete P; return rc; }
    *out = P;
    return GEMHIP_OK;
}

extern "C" int gemhip_hope_plan_destroy(gemhip_hope_plan_t P)
{
    delete P;
    return GEMHIP_OK;
}

extern "C" int gemhip_hope_plan_solve(gemhip_hope_plan_t P, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol,
                                      uint64_t seed, float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats)
{
    GEMHIP_REQUIRE(P != nullptr, "hope_plan_solve: NULL plan");
    GEMHIP_REQUIRE(k >= 1 && k < P->H.n, "hope: k=%d must satisfy 1 <= k < n=%lld (svds requirement)", k, (long long)P->H.n);
    GEMHIP_REQUIRE(U_sqrtS && V_sqrtS && sigma, "hope: output pointers are NULL");
    GEMHIP_REQUIRE(oversample >= 0 && krylov_steps >= 1 && max_restarts >= 0, "hope: need oversample >= 0, krylov_steps >= 1, max_restarts >= 0");
    return solve_operator(P->H, P->symmetric && P->H.beta > 0.f, k, oversample, krylov_steps, max_restarts, tol, seed, P->terms, P->br, 0, U_sqrtS, V_sqrtS, sigma, stats);
}

// The same solve with U sqrt(S) and V sqrt(S) left in device memory (n x k floats each, row-major; sigma and stats stay host pointers): for callers
// that keep the embedding in HBM (evaluation on the device, a following GPU stage) -- the two 4nk-byte PCIe copies into pageable host memory are
// 1.9 ms of a 13.5 ms solve at n = 100k, k = 64.  The output copies above use hipMemcpyDefault, so this is the same code path.
extern "C" int gemhip_hope_plan_solve_device(gemhip_hope_plan_t P, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol,
                                             uint64_t seed, void *dU_sqrtS, void *dV_sqrtS, float *sigma, double *stats)
{
    GEMHIP_REQUIRE(dU_sqrtS && dV_sqrtS, "hope_plan_solve_device: output pointers are NULL");
    auto on_device = [](const void *p) {
        hipPointerAttribute_t a;
        const bool ok = hipPointerGetAttributes(&a, p) == hipSuccess && a.type == hipMemoryTypeDevice;
        (void)hipGetLastError();            // a plain host pointer makes the query itself fail: do not leave that error for the next launch check
        return ok;
    };
    GEMHIP_REQUIRE(on_device(dU_sqrtS) && on_device(dV_sqrtS),
                   "hope_plan_solve_device: U / V must be device pointers (use gemhip_hope_plan_solve for host buffers)");
    return gemhip_hope_plan_solve(P, k, oversample, krylov_steps, max_restarts, tol, seed, (float *)dU_sqrtS, (float *)dV_sqrtS, sigma, stats);
}

extern "C" int gemhip_hope(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, int32_t k,
                           int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed, float *U_sqrtS,
                           float *V_sqrtS, float *sigma, double *stats)
{
    for (int q = 0; q < PH_COUNT; ++q) phase_acc()[q] = 0.0;
    const double t_call = phase_now();
    gemhip_hope_plan_t P = nullptr;
    int rc = gemhip_hope_plan_create(n, nnz, row_ptr, col, w, beta, &P);
    if (rc) return rc;
    // gemhip_last_call_phases: the plan (transpose, symmetry test, uploads, spectral-radius estimate) counts as host preparation as a whole;
    // kernel_seconds = the solver's own figure (stats[0]: device work and the projected host eigensolves between them), the rest of the solve
    // call is the two n x k outputs reaching the caller's pageable buffers
    const double t_solve = phase_now();
    phase_acc()[PH_HOST] = t_solve - t_call;
    double st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    rc = gemhip_hope_plan_solve(P, k, oversample, krylov_steps, max_restarts, tol, seed, U_sqrtS, V_sqrtS, sigma, st);
    if (stats) for (int q = 0; q < 12; ++q) stats[q] = st[q];
    const double t_done = phase_now();
    phase_acc()[PH_KERNELS] = st[0];
    phase_acc()[PH_D2H] = std::max(0.0, (t_done - t_solve) - st[0]);
    gemhip_hope_plan_destroy(P);
    phase_acc()[PH_TOTAL] = phase_now() - t_call;
    return rc;
}

// hope.py:38-40 prints `SVD error (low rank): ||u diag(s) vt - S||_F` from the dense S it formed.  For the exact truncated SVD that matrix is
// S (I - V V^T), V = the k right singular vectors, so the number is ||S P||_F with P the projector onto V's complement, and
// ||S P||_F^2 = E ||S P z||^2 over z ~ N(0, I) (Hutchinson): the Katz series applied to `probes` random columns with the SpMM kernel the solve itself
// uses.  Two things keep the variance down.  (1) The probes are deflated (z - V V^T z): the dominant singular directions, which carry most of
// ||S||_F^2 and all of a plain estimate's variance, never enter.  (2) S = B + B^2 + ... with B = beta A, and ||B P||_F^2 = ||B||_F^2 - ||B V||_F^2 is
// known exactly (beta^2 sum w^2 and one SpMM on V), so the probes only estimate the remainder: err^2 ~ ||B P||_F^2 + mean_z (||S P z||^2 - ||B P z||^2).
// On the reference's graphs (beta x degree << 1) the result is good to a few 1e-3 relative with 32 probes (tests/test_run_sbm_gpu.py: dense value).
// sigma / V_sqrtS: what a solve returned (V sqrt(Sigma), n x k row-major, host).  frob2_out (optional): err^2 + sum sigma^2 = ||S||_F^2.
// U_sqrtS (optional, round 6 -- ADVICE r5): with it the U side of the factorisation enters.  For orthonormal V,
//   u diag(s) vt - S = (U Sigma - S V) V^T - S (I - V V^T),  the two terms orthogonal in the Frobenius inner product ((I - V V^T) V = 0),
// so ||u diag(s) vt - S||_F^2 = ||S (I - V V^T)||_F^2 + ||S V - U Sigma||_F^2: the second term is computed EXACTLY (the Katz series applied to V's k
// columns, U Sigma subtracted on the device, one Gram trace) and is ~0 for a converged solve -- a wrong or unconverged U now shows in the print, as it does in
// the reference's.  Without U the result is the truncation error of an exact SVD with this V.  Columns with sigma[j] <= 0 (k above the rank of S) carry no
// direction: they are skipped on both sides instead of failing.
static int svd_error_impl(gemhip_hope_plan_t P, int32_t k, const float *sigma, const float *U_sqrtS, const float *V_sqrtS, int32_t probes, uint64_t seed,
                          double *err_out, double *frob2_out, double *uside_out)
{
    GEMHIP_REQUIRE(P != nullptr && sigma != nullptr && V_sqrtS != nullptr && err_out != nullptr && k >= 1 && k <= 512, "hope_plan_svd_error: bad arguments (1 <= k <= 512)");
    GEMHIP_REQUIRE(probes >= 1 && probes <= 128, "hope_plan_svd_error: probes=%d (1..128)", probes);
    Hope &H = P->H;
    GEMHIP_REQUIRE(H.mode == 0, "hope_plan_svd_error: the plan is not a Katz (HOPE) operator");
    H.err = 0;
    const int64_t n = H.n;
    const int ld = (probes + 31) / 32 * 32, ldv = (k + 31) / 32 * 32;
    // unit right singular vectors, padded to the MFMA tile width
    std::vector<float> Vh((size_t)n * ldv, 0.f);
    for (int j = 0; j < k; ++j) GEMHIP_REQUIRE(std::isfinite(sigma[j]), "hope_plan_svd_error: sigma[%d] = %g", j, (double)sigma[j]);
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) Vh[(size_t)i * ldv + j] = sigma[j] > 0.f ? V_sqrtS[(size_t)i * k + j] / std::sqrt(sigma[j]) : 0.f;      // (a zero column deflates nothing)
    DevBuf<float> dV, dBV;
    DevBuf<float> blk[5];                                                    // Z (deflated in place), T0, T1, W0 (= B Z after apply_S), Out (= S Z)
    HOPE_TRY(H, dV.reserve(Vh.size()));
    HOPE_TRY(H, dBV.reserve(Vh.size()));
    for (DevBuf<float> &b : blk) { HOPE_TRY(H, b.reserve((size_t)n * ld)); HOPE_TRY(H, hipMemsetAsync(b, 0, (size_t)n * ld * sizeof(float), H.s)); }
    HOPE_TRY(H, hipMemcpyAsync(dV, Vh.data(), Vh.size() * sizeof(float), hipMemcpyHostToDevice, H.s));
    HOPE_TRY(H, hipMemsetAsync(dBV, 0, Vh.size() * sizeof(float), H.s));
    std::vector<double> Gbv, C, Gs, Gb;
    if (!H.err) {
        for (int c0 = 0; c0 < k; c0 += 128) {                                  // B V, at most 128 columns per SpMM launch
            const int cb = std::min(128, k - c0);
            spmm(H, false, H.beta, dV + c0, ldv, nullptr, 0, dBV + c0, ldv, cb);
        }
        gram(H, dBV, ldv, k, dBV, ldv, k, Gbv);
        randn(H, blk[0], probes, ld, seed ^ 0x5356444572726F72ull);
        gram(H, dV, ldv, k, blk[0], ld, probes, C);                            // V^T Z  (k x probes)
        tsgemm(H, dV, ldv, k, C, probes, -1.0f, blk[0], ld, blk[0], ld);       // Z <- Z - V (V^T Z)
        apply_S(H, blk[0], ld, probes, P->terms, blk[1], blk[2], blk[3], ld, blk[4], ld);           // W0 keeps the first term B Z
        gram(H, blk[4], ld, probes, blk[4], ld, probes, Gs);
        gram(H, blk[3], ld, probes, blk[3], ld, probes, Gb);
    }
    // the U side: ||S V - U Sigma||_F^2, at most 128 columns of V per pass of the Katz series
    double uside = 0.0;
    if (U_sqrtS && !H.err) {
        const int ldc = 128;
        DevBuf<float> cb[5];                                               // T0, T1, W0, Out (= S V chunk), U Sigma chunk / residual
        for (DevBuf<float> &b : cb) HOPE_TRY(H, b.reserve((size_t)n * ldc));
        std::vector<float> Uh((size_t)n * ldc);
        for (int c0 = 0; c0 < k && !H.err; c0 += ldc) {
            const int cbn = std::min(ldc, k - c0);
            std::fill(Uh.begin(), Uh.end(), 0.f);
            for (int64_t i = 0; i < n; ++i)
                for (int j = 0; j < cbn; ++j) Uh[(size_t)i * ldc + j] = sigma[c0 + j] > 0.f ? U_sqrtS[(size_t)i * k + c0 + j] * std::sqrt(sigma[c0 + j]) : 0.f;
            HOPE_TRY(H, hipMemcpyAsync(cb[4], Uh.data(), Uh.size() * sizeof(float), hipMemcpyHostToDevice, H.s));
            HOPE_TRY(H, hipMemsetAsync(cb[3], 0, (size_t)n * ldc * sizeof(float), H.s));
            apply_S(H, dV + c0, ldv, cbn, P->terms, cb[0], cb[1], cb[2], ldc, cb[3], ldc);
            lincomb(H, ldc, 1.0f, cb[3], ldc, -1.0f, cb[4], ldc, 0.0f, cb[4], ldc, cb[4], ldc);      // residual in place (padding columns: 0 - 0)
            std::vector<double> Gr;
            const int cpad = (cbn + 31) / 32 * 32;
            gram(H, cb[4], ldc, cpad, cb[4], ldc, cpad, Gr);
            HOPE_TRY(H, hipStreamSynchronize(H.s));
            if (!H.err) for (int j = 0; j < cbn; ++j) uside += Gr[(size_t)j * cpad + j];
        }
    }
    HOPE_TRY(H, hipStreamSynchronize(H.s));
    if (H.err) return H.err;
    double rem = 0.0, bv2 = 0.0, top = 0.0;
    for (int j = 0; j < probes; ++j) rem += Gs[(size_t)j * probes + j] - Gb[(size_t)j * probes + j];
    for (int j = 0; j < k; ++j) { bv2 += Gbv[(size_t)j * k + j]; top += (double)sigma[j] * (double)sigma[j]; }
    const double trunc2 = std::max(0.0, (double)H.beta * (double)H.beta * P->frob2_A - bv2 + rem / probes);
    const double err2 = trunc2 + std::max(0.0, uside);
    *err_out = std::sqrt(err2);
    if (frob2_out) *frob2_out = trunc2 + top;
    if (uside_out) *uside_out = std::sqrt(std::max(0.0, uside));
    return GEMHIP_OK;
}

extern "C" int gemhip_hope_plan_svd_error(gemhip_hope_plan_t P, int32_t k, const float *sigma, const float *V_sqrtS, int32_t probes, uint64_t seed,
                                          double *err_out, double *frob2_out)
{
    return svd_error_impl(P, k, sigma, nullptr, V_sqrtS, probes, seed, err_out, frob2_out, nullptr);
}

extern "C" int gemhip_hope_plan_svd_error_uv(gemhip_hope_plan_t P, int32_t k, const float *sigma, const float *U_sqrtS, const float *V_sqrtS, int32_t probes,
                                             uint64_t seed, double *err_out, double *frob2_out, double *uside_out)
{
    GEMHIP_REQUIRE(U_sqrtS != nullptr, "hope_plan_svd_error_uv: U_sqrtS is NULL (gemhip_hope_plan_svd_error is the V-only form)");
    return svd_error_impl(P, k, sigma, U_sqrtS, V_sqrtS, probes, seed, err_out, frob2_out, uside_out);
}

extern "C" int gemhip_hope_svd_error_uv(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, int32_t k,
                                        const float *sigma, const float *U_sqrtS, const float *V_sqrtS, int32_t probes, uint64_t seed, double *err_out,
                                        double *frob2_out, double *uside_out)
{
    gemhip_hope_plan_t P = nullptr;
    int rc = gemhip_hope_plan_create(n, nnz, row_ptr, col, w, beta, &P);
    if (rc) return rc;
    rc = gemhip_hope_plan_svd_error_uv(P, k, sigma, U_sqrtS, V_sqrtS, probes, seed, err_out, frob2_out, uside_out);
    gemhip_hope_plan_destroy(P);
    return rc;
}

// One-shot form for the plugin's verbose mode (hope.py:38-40): the plan is rebuilt (transpose + uploads), which costs about as much as the estimate itself.
extern "C" int gemhip_hope_svd_error(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, int32_t k,
                                     const float *sigma, const float *V_sqrtS, int32_t probes, uint64_t seed, double *err_out, double *frob2_out)
{
    gemhip_hope_plan_t P = nullptr;
    int rc = gemhip_hope_plan_create(n, nnz, row_ptr, col, w, beta, &P);
    if (rc) return rc;
    rc = gemhip_hope_plan_svd_error(P, k, sigma, V_sqrtS, probes, seed, err_out, frob2_out);
    gemhip_hope_plan_destroy(P);
    return rc;
}

// ------------------------------------------------------------------ Laplacian Eigenmaps
// gem/embedding/lap.py:21-37: w, v = eigs(normalized_laplacian(graph.to_undirected()), k=d+1, which='SM'); X = v[:, 1:].
// The d+1 SMALLEST eigenpairs of L_sym = I - D^-1/2 A D^-1/2 are the d+1 LARGEST of T = I + D^-1/2 A D^-1/2 (symmetric,
// positive semi-definite, eigenvalue 2 - w): same block-Krylov machinery, one SpMM per operator application.
// Input: CSR of the SYMMETRIC weighted adjacency; the normalisation is done here.  eigvals: the k smallest eigenvalues of
// L_sym ascending; V_out [n][k] unit eigenvectors in that order (column 0 = the trivial one lap.py drops).
extern "C" int gemhip_lap_eigmap(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t k, int32_t oversample,
                                 int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed, float *V_out, float *eigvals, double *stats)
{
    if (const int rc = check_csr("lap_eigmap", n, nnz, row_ptr, col)) return rc;
    GEMHIP_REQUIRE(k >= 1 && k < n && V_out && eigvals, "lap_eigmap: need 1 <= k < n and output buffers");
    GEMHIP_REQUIRE(oversample >= 0 && krylov_steps >= 1 && max_restarts >= 0, "lap_eigmap: bad solver parameters");
    Hope H; H.beta = 1.0f; H.mode = 1;
    std::vector<float> va(std::max<int64_t>(nnz, 1));
    lap_edge_values(n, row_ptr, col, w, va.data());
    if (upload_csr(H, "lap_eigmap", n, nnz, row_ptr, col, va.data(), nullptr)) return H.err;
    std::vector<float> sig(k);
    if (const int rc = solve_operator(H, true, k, oversample, krylov_steps, max_restarts, tol, seed, 0, 0.0, 1, nullptr, V_out, sig.data(), stats)) return rc;
    // sigma ascending = (2 - w) ascending; lap.py wants w ascending: reverse the columns
    for (int j = 0; j < k; ++j) eigvals[j] = 2.0f - sig[k - 1 - j];
    reverse_columns(V_out, n, k);
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ Locally Linear Embedding
// gem/embedding/lle.py:23-35: A row-normalised (l1), u, s, vt = svds(I - A, k=d+1, which='SM'); X = vt.T[:, 1:].
// The d+1 smallest right singular vectors of N = I - P are the d+1 largest eigenvectors of c I - N^T N
// (c >= sigma_max(N)^2), a symmetric PSD operator: two SpMMs (P, P^T) per application on the same block-Krylov core.
// Input: CSR of the SYMMETRIC weighted adjacency in graph.nodes order; rows are l1-normalised here.
// sing[k]: the k smallest singular values of I - P ascending; V_out [n][k] the matching right singular vectors.
extern "C" int gemhip_lle(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t k, int32_t oversample,
                          int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed, float *V_out, float *sing, double *stats)
{
    if (const int rc = check_csr("lle", n, nnz, row_ptr, col)) return rc;
    GEMHIP_REQUIRE(k >= 1 && k < n && V_out && sing, "lle: need 1 <= k < n and output buffers");
    GEMHIP_REQUIRE(oversample >= 0 && krylov_steps >= 1 && max_restarts >= 0, "lle: bad solver parameters");
    Hope H; H.mode = 2;
    std::vector<float> va(std::max<int64_t>(nnz, 1));
    lle_edge_values(n, row_ptr, w, va.data());
    const CsrT T = transpose_csr(n, nnz, row_ptr, col, va.data());
    if (upload_csr(H, "lle", n, nnz, row_ptr, col, va.data(), &T)) return H.err;
    // c >= sigma_max(I - P)^2 by power iteration on N^T N (at most 60 steps), with a 5 % margin
    const double est = power_iteration(H, 0.61, 7.31, 60, 8, 1e-4, false, [&](float *X2, float *t) {
        apply_sym_op(H, 2, 1.0f, X2, 2, 1, t, 1, X2 + 1, 2, 1.0f, nullptr, 0, 0.f, nullptr, 0);            // z = N^T N x
    });
    if (H.err) return H.err;
    const double c = est > 0.0 ? est * 1.05 : 4.0;
    H.beta = (float)c;
    std::vector<float> sig(k);
    // (large graphs: the Chebyshev-filtered eigen-path on N^T N itself (kind 2), which converges where the block-Krylov solver runs out of its
    // restart budget -- the bottom of the spectrum is clustered)
    if (const int rc = solve_operator(H, true, k, oversample, krylov_steps, max_restarts, tol, seed, 0, 0.0, 1, nullptr, V_out, sig.data(), stats)) return rc;
    // eigenvalue of c I - N^T N = c - s^2 (ascending in sig) -> s ascending means reversing the columns
    for (int j = 0; j < k; ++j) sing[j] = (float)std::sqrt(std::max(c - (double)sig[k - 1 - j], 0.0));
    reverse_columns(V_out, n, k);
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ building blocks, exposed for kernel-level parity tests
extern "C" int gemhip_set_sym_eig_callback(int (*fn)(int32_t, double *, double *)) { set_sym_eig_callback(fn); return GEMHIP_OK; }

extern "C" int gemhip_set_host_threads(int32_t threads, int32_t *in_effect_out)
{
    GEMHIP_REQUIRE(threads <= 16, "set_host_threads: at most 16 threads (got %d)", threads);
    set_eig_threads(threads);                       // <= 0: back to the default
    const int t = eig_threads_in_effect();
    if (in_effect_out) *in_effect_out = t;
    return GEMHIP_OK;
}

static int sym_eig_full(const char *who, void (*solver)(int, std::vector<double> &, std::vector<double> &), int32_t n, double *A_inout, double *w_out)
{
    GEMHIP_REQUIRE(n >= 1 && A_inout && w_out, "%s: bad arguments", who);
    std::vector<double> V(A_inout, A_inout + (size_t)n * n), w;
    solver(n, V, w);
    std::copy(V.begin(), V.end(), A_inout);
    std::copy(w.begin(), w.end(), w_out);
    return GEMHIP_OK;
}
extern "C" int gemhip_sym_eig_builtin(int32_t n, double *A_inout, double *w_out) { return sym_eig_full("sym_eig_builtin", sym_eig_impl, n, A_inout, w_out); }
extern "C" int gemhip_sym_eig(int32_t n, double *A_inout, double *w_out) { return sym_eig_full("sym_eig", sym_eig, n, A_inout, w_out); }

extern "C" int gemhip_sym_eig_top(int32_t n, double *A_inout, int32_t m, double *w_out, double *Z_out)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && m <= n && A_inout && w_out && Z_out, "sym_eig_top: bad arguments");
    std::vector<double> V(A_inout, A_inout + (size_t)n * n), w, Z;
    sym_eig_top_impl(n, V, m, w, Z);
    std::copy(w.begin(), w.end(), w_out);
    std::copy(Z.begin(), Z.end(), Z_out);
    return GEMHIP_OK;
}

extern "C" int gemhip_hope_spmm(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float alpha, int32_t b,
                                const float *X_host, const float *Wadd_host, float *Y_host)
{
    GEMHIP_REQUIRE(n >= 1 && row_ptr && X_host && Y_host && b >= 1 && b <= 512, "hope_spmm: bad arguments");
    Hope H;
    DevBuf<float> dX, dW, dY;
    upload_csr_w(H, n, nnz, row_ptr, col, w, false);
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * b));
    if (Wadd_host) HOPE_TRY(H, dW.upload(Wadd_host, (size_t)n * b));
    HOPE_TRY(H, dY.reserve((size_t)n * b));
    spmm(H, false, alpha, dX, b, dW, b, dY, b, b);
    HOPE_TRY(H, hipMemcpy(Y_host, dY, (size_t)n * b * 4, hipMemcpyDeviceToHost));
    return H.err;
}

extern "C" int gemhip_hope_gram(int64_t n, int32_t m1, int32_t m2, const float *X_host, const float *Y_host, double *G_host)
{
    GEMHIP_REQUIRE(n >= 1 && m1 >= 1 && m2 >= 1 && X_host && Y_host && G_host, "hope_gram: bad arguments");
    Hope H; H.n = n;
    DevBuf<float> dX, dY;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * m1)); HOPE_TRY(H, dY.upload(Y_host, (size_t)n * m2));
    std::vector<double> G;
    gram(H, dX, m1, m1, dY, m2, m2, G);
    if (!H.err) std::copy(G.begin(), G.end(), G_host);
    return H.err;
}

extern "C" int gemhip_hope_tsgemm(int64_t n, int32_t m, int32_t b2, const float *X_host, const double *C_host, float alpha, const float *Src_host,
                                  float *Out_host)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && b2 >= 1 && X_host && C_host && Out_host, "hope_tsgemm: bad arguments");
    Hope H; H.n = n;
    DevBuf<float> dX, dS, dO;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * m));
    if (Src_host) HOPE_TRY(H, dS.upload(Src_host, (size_t)n * b2));
    HOPE_TRY(H, dO.reserve((size_t)n * b2));
    std::vector<double> C(C_host, C_host + (size_t)m * b2);
    tsgemm(H, dX, m, m, C, b2, alpha, dS, b2, dO, b2);
    HOPE_TRY(H, hipMemcpy(Out_host, dO, (size_t)n * b2 * 4, hipMemcpyDeviceToHost));
    return H.err;
}

// ------------------------------------------------------------------ test hooks: the host functions above, under the solvers' calling conventions
// Each hook uploads host blocks (every one with its full leading dimension, padding included), calls the host function the solvers call on a local
// Hope, and copies the output block back whole, so a caller that filled the padding with a sentinel sees any write outside the logical columns.
namespace {

bool hook_csr_ok(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col)
{
    if (n < 1 || nnz < 0 || !row_ptr || (nnz > 0 && !col) || row_ptr[0] != 0 || row_ptr[n] != nnz) return false;
    for (int64_t i = 0; i < n; ++i) if (row_ptr[i + 1] < row_ptr[i]) return false;
    for (int64_t e = 0; e < nnz; ++e) if (col[e] < 0 || col[e] >= n) return false;
    return true;
}

int hook_download(Hope &H, void *host, const void *dev, size_t bytes)      // blocking: the null stream's work is done when it returns
{
    HOPE_TRY(H, hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return H.err;
}

}  // namespace

// variant: 0 = the production dispatch, 1 = hope_spmm_kernel (one row per wavefront), 2 / 4 / 8 = hope_spmm16_kernel with that U.
// w_is_x: Wadd is the device block of X itself (ldw = ldx); w2_is_y: W2 is the device block of Y itself (Y_inout's contents, ldw2 = ldy).
// launched_out (may be NULL): the instantiation spmm() chose, {CPL16, U} or {CPL, 0}.
extern "C" int gemhip_test_hope_spmm(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t variant, float alpha,
                                     int32_t b, const float *X_host, int32_t ldx, float wa, const float *W_host, int32_t ldw, float wb,
                                     const float *W2_host, int32_t ldw2, int32_t w_is_x, int32_t w2_is_y, float *Y_inout, int32_t ldy,
                                     int32_t *launched_out)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_spmm: bad CSR arguments");
    GEMHIP_REQUIRE(X_host && Y_inout && b >= 1 && b <= 512 && ldx >= b && ldy >= b, "test_hope_spmm: bad block arguments");
    GEMHIP_REQUIRE(variant == 0 || variant == 1 || ((variant == 2 || variant == 4 || variant == 8) && b <= 128), "test_hope_spmm: variant %d", variant);
    GEMHIP_REQUIRE(!(w_is_x && W_host) && !(w2_is_y && W2_host) && (!W_host || ldw >= b) && (!W2_host || ldw2 >= b), "test_hope_spmm: bad addend arguments");
    Hope H;
    upload_csr_w(H, n, nnz, row_ptr, col, w, false);
    if (variant == 1) H.force_spmm16 = 0;
    if (variant >= 2) { H.force_spmm16 = 1; H.force_spmm16_u = variant; }
    DevBuf<float> dX, dW, dW2, dY;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * ldx));
    if (W_host) HOPE_TRY(H, dW.upload(W_host, (size_t)n * ldw));
    if (W2_host) HOPE_TRY(H, dW2.upload(W2_host, (size_t)n * ldw2));
    HOPE_TRY(H, dY.upload(Y_inout, (size_t)n * ldy));
    const float *pW = w_is_x ? dX.get() : dW.get(); const int lw = w_is_x ? ldx : ldw;
    const float *pW2 = w2_is_y ? dY.get() : dW2.get(); const int lw2 = w2_is_y ? ldy : ldw2;
    spmm(H, false, alpha, dX, ldx, pW, lw, dY, ldy, b, wa, pW2, lw2, wb);
    if (launched_out) { launched_out[0] = H.last_spmm_c; launched_out[1] = H.last_spmm_u; }
    return hook_download(H, Y_inout, dY, (size_t)n * ldy * sizeof(float));
}

// G[m1][m2] = X[:, xoff : xoff + m1]^T Y[:, yoff : yoff + m2]; Y_host NULL: Y is the device block of X (ldy = ldx).  Gf_host (may be NULL) receives
// the fp32 rounding hope_reduce2_kernel writes for project_out.
extern "C" int gemhip_test_hope_gram(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m1, const float *Y_host, int32_t ldy, int32_t yoff,
                                     int32_t m2, double *G_host, float *Gf_host)
{
    GEMHIP_REQUIRE(n >= 1 && X_host && G_host && m1 >= 1 && m2 >= 1 && xoff >= 0 && yoff >= 0 && xoff + m1 <= ldx && yoff + m2 <= (Y_host ? ldy : ldx),
                   "test_hope_gram: bad arguments");
    Hope H; H.n = n;
    DevBuf<float> dX, dY, dGf;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * ldx));
    if (Y_host) HOPE_TRY(H, dY.upload(Y_host, (size_t)n * ldy));
    const float *pY = Y_host ? dY.get() : dX.get(); const int ly = Y_host ? ldy : ldx;
    if (!Gf_host) {
        std::vector<double> G;
        gram(H, dX + xoff, ldx, m1, pY + yoff, ly, m2, G);
        if (!H.err) std::copy(G.begin(), G.end(), G_host);
        return H.err;
    }
    HOPE_TRY(H, dGf.reserve((size_t)m1 * m2));
    gram_launch(H, dX + xoff, ldx, m1, pY + yoff, ly, m2, dGf);
    if (hook_download(H, G_host, H.G, (size_t)m1 * m2 * sizeof(double))) return H.err;
    return hook_download(H, Gf_host, dGf, (size_t)m1 * m2 * sizeof(float));
}

// gram2: Ga = Xa[:, xaoff : +ma1]^T Ya[:, yaoff : +ma2] and Gb likewise, in one call (shared scratch, one host round trip)
extern "C" int gemhip_test_hope_gram2(int64_t n, const float *Xa_host, int32_t ldxa, int32_t xaoff, int32_t ma1, const float *Ya_host, int32_t ldya,
                                      int32_t yaoff, int32_t ma2, double *Ga_host, const float *Xb_host, int32_t ldxb, int32_t xboff, int32_t mb1,
                                      const float *Yb_host, int32_t ldyb, int32_t yboff, int32_t mb2, double *Gb_host)
{
    GEMHIP_REQUIRE(n >= 1 && Xa_host && Ya_host && Xb_host && Yb_host && Ga_host && Gb_host, "test_hope_gram2: NULL argument");
    GEMHIP_REQUIRE(ma1 >= 1 && ma2 >= 1 && mb1 >= 1 && mb2 >= 1 && xaoff >= 0 && yaoff >= 0 && xboff >= 0 && yboff >= 0 && xaoff + ma1 <= ldxa &&
                   yaoff + ma2 <= ldya && xboff + mb1 <= ldxb && yboff + mb2 <= ldyb, "test_hope_gram2: bad shapes");
    Hope H; H.n = n;
    DevBuf<float> dXa, dYa, dXb, dYb;
    HOPE_TRY(H, dXa.upload(Xa_host, (size_t)n * ldxa)); HOPE_TRY(H, dYa.upload(Ya_host, (size_t)n * ldya));
    HOPE_TRY(H, dXb.upload(Xb_host, (size_t)n * ldxb)); HOPE_TRY(H, dYb.upload(Yb_host, (size_t)n * ldyb));
    std::vector<double> Ga, Gb;
    gram2(H, dXa + xaoff, ldxa, ma1, dYa + yaoff, ldya, ma2, Ga, dXb + xboff, ldxb, mb1, dYb + yboff, ldyb, mb2, Gb);
    if (!H.err) { std::copy(Ga.begin(), Ga.end(), Ga_host); std::copy(Gb.begin(), Gb.end(), Gb_host); }
    return H.err;
}

// Out[:, :b2] = (Src or 0) + alpha X[:, xoff : xoff + m] C.  in_place: Src is the device block of Out (Out_inout's contents, lds = ldo).
extern "C" int gemhip_test_hope_tsgemm(int64_t n, const float *X_host, int32_t ldx, int32_t xoff, int32_t m, const double *C_host, int32_t b2, float alpha,
                                       const float *Src_host, int32_t lds, int32_t in_place, float *Out_inout, int32_t ldo)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && b2 >= 1 && X_host && C_host && Out_inout && xoff >= 0 && xoff + m <= ldx && ldo >= b2, "test_hope_tsgemm: bad arguments");
    GEMHIP_REQUIRE(!(in_place && Src_host) && (!Src_host || lds >= b2), "test_hope_tsgemm: bad Src arguments");
    Hope H; H.n = n;
    DevBuf<float> dX, dS, dO;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * ldx));
    if (Src_host) HOPE_TRY(H, dS.upload(Src_host, (size_t)n * lds));
    HOPE_TRY(H, dO.upload(Out_inout, (size_t)n * ldo));
    std::vector<double> C(C_host, C_host + (size_t)m * b2);
    tsgemm(H, dX + xoff, ldx, m, C, b2, alpha, in_place ? dO.get() : dS.get(), in_place ? ldo : lds, dO, ldo);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// ritz_rotate: Out[:, :b2] = V[:, voff : +m] C, res2[j] = || B[:, boff : +m] C[:, j] - theta[j] Out[:, j] ||^2
extern "C" int gemhip_test_hope_ritz(int64_t n, const float *V_host, int32_t ldv, int32_t voff, const float *B_host, int32_t ldb, int32_t boff, int32_t m,
                                     const double *C_host, const double *theta_host, int32_t b2, float *Out_inout, int32_t ldo, double *res2_out)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 1 && b2 >= 1 && V_host && B_host && C_host && theta_host && Out_inout && res2_out, "test_hope_ritz: bad arguments");
    GEMHIP_REQUIRE(voff >= 0 && boff >= 0 && voff + m <= ldv && boff + m <= ldb && ldo >= b2, "test_hope_ritz: bad shapes");
    Hope H; H.n = n;
    DevBuf<float> dV, dB, dO;
    HOPE_TRY(H, dV.upload(V_host, (size_t)n * ldv)); HOPE_TRY(H, dB.upload(B_host, (size_t)n * ldb)); HOPE_TRY(H, dO.upload(Out_inout, (size_t)n * ldo));
    const std::vector<double> C(C_host, C_host + (size_t)m * b2), theta(theta_host, theta_host + b2);
    std::vector<double> res2;
    ritz_rotate(H, dV + voff, ldv, dB + boff, ldb, m, C, theta, b2, dO, ldo, res2);
    if (!H.err) std::copy(res2.begin(), res2.end(), res2_out);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// colmax: val[j] = the entry of X[:, j] (j < mc) with the largest magnitude, first row on ties.  variant: 0 = production choice, 1 = one pass
// (hope_colmax_kernel), 2 = two passes (hope_colmax1/2_kernel).
extern "C" int gemhip_test_hope_colmax(int64_t n, const float *X_host, int32_t ld, int32_t mc, int32_t variant, float *val_out)
{
    GEMHIP_REQUIRE(n >= 1 && X_host && val_out && mc >= 1 && ld >= mc && variant >= 0 && variant <= 2, "test_hope_colmax: bad arguments");
    Hope H; H.n = n;
    if (variant) H.force_colmax2 = variant - 1;
    DevBuf<float> dX, dv;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * ld));
    HOPE_TRY(H, dv.reserve(mc));
    colmax(H, dX, ld, mc, dv);
    return hook_download(H, val_out, dv, (size_t)mc * sizeof(float));
}

// project_out: W[:, :cols] -= V[:, :m] (V[:, :m]^T W[:, :cols]).  woff < 0: W_inout is its own n x ldw block.  woff >= 0: as in the solvers, W is the
// column block [woff, woff + cols) of V's own block (W = V + woff, ldw = ldv) and W_inout (n x ldv) receives that whole block back.
extern "C" int gemhip_test_hope_project_out(int64_t n, const float *V_host, int32_t ldv, int32_t m, float *W_inout, int32_t ldw, int32_t cols, int32_t woff)
{
    GEMHIP_REQUIRE(n >= 1 && V_host && W_inout && m >= 1 && cols >= 1 && m <= ldv && cols <= ldw, "test_hope_project_out: bad arguments");
    GEMHIP_REQUIRE(woff < 0 || (woff >= m && woff + cols <= ldv && ldw == ldv), "test_hope_project_out: bad shared block");
    Hope H; H.n = n;
    DevBuf<float> dV, dW;
    HOPE_TRY(H, dV.upload(V_host, (size_t)n * ldv));
    if (woff < 0) HOPE_TRY(H, dW.upload(W_inout, (size_t)n * ldw));
    project_out(H, dV, ldv, m, woff < 0 ? dW.get() : dV.get() + woff, ldw, cols);
    return hook_download(H, W_inout, woff < 0 ? dW.get() : dV.get(), (size_t)n * ldw * sizeof(float));
}

// apply_sym_op: Out[:, :cols] = alpha Op X + wa W + wb W2; kind 0: Op = the CSR matrix, kind 2: Op = (I - A)^T (I - A) (A as given: the caller
// normalises the rows).  The n x cols scratch of kind 2 is the hook's own.
extern "C" int gemhip_test_hope_sym_op(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t kind, float alpha,
                                       const float *X_host, int32_t ldx, int32_t cols, float wa, const float *W_host, int32_t ldw, float wb,
                                       const float *W2_host, int32_t ldw2, float *Out_inout, int32_t ldo)
{
    GEMHIP_REQUIRE(hook_csr_ok(n, nnz, row_ptr, col), "test_hope_sym_op: bad CSR arguments");
    GEMHIP_REQUIRE((kind == 0 || kind == 2) && X_host && Out_inout && cols >= 1 && cols <= 512 && ldx >= cols && ldo >= cols, "test_hope_sym_op: bad arguments");
    GEMHIP_REQUIRE((!W_host || ldw >= cols) && (!W2_host || ldw2 >= cols), "test_hope_sym_op: bad addend arguments");
    Hope H;
    upload_csr_w(H, n, nnz, row_ptr, col, w, true);
    H.mode = kind;
    DevBuf<float> dX, dW, dW2, dT, dO;
    HOPE_TRY(H, dX.upload(X_host, (size_t)n * ldx));
    if (W_host) HOPE_TRY(H, dW.upload(W_host, (size_t)n * ldw));
    if (W2_host) HOPE_TRY(H, dW2.upload(W2_host, (size_t)n * ldw2));
    HOPE_TRY(H, dT.reserve((size_t)n * cols));
    HOPE_TRY(H, dO.upload(Out_inout, (size_t)n * ldo));
    apply_sym_op(H, kind, alpha, dX, ldx, cols, dT, cols, dO, ldo, wa, dW, ldw, wb, dW2, ldw2);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// lincomb: Out[:, :b] = a X + b2 Y + c Z.  out_is_x: Out is the device block of X (Out_inout's contents are X, ldx = ldo; X_host NULL).
extern "C" int gemhip_test_hope_lincomb(int64_t n, int32_t b, float a, const float *X_host, int32_t ldx, float b2, const float *Y_host, int32_t ldy, float c,
                                        const float *Z_host, int32_t ldz, int32_t out_is_x, float *Out_inout, int32_t ldo)
{
    GEMHIP_REQUIRE(n >= 1 && b >= 1 && Y_host && Z_host && Out_inout && ldy >= b && ldz >= b && ldo >= b, "test_hope_lincomb: bad arguments");
    GEMHIP_REQUIRE(out_is_x ? X_host == nullptr : (X_host != nullptr && ldx >= b), "test_hope_lincomb: X_host and out_is_x exclude each other");
    Hope H; H.n = n;
    DevBuf<float> dX, dY, dZ, dO;
    if (X_host) HOPE_TRY(H, dX.upload(X_host, (size_t)n * ldx));
    HOPE_TRY(H, dY.upload(Y_host, (size_t)n * ldy)); HOPE_TRY(H, dZ.upload(Z_host, (size_t)n * ldz));
    HOPE_TRY(H, dO.upload(Out_inout, (size_t)n * ldo));
    lincomb(H, b, a, out_is_x ? dO.get() : dX.get(), out_is_x ? ldo : ldx, b2, dY, ldy, c, dZ, ldz, dO, ldo);
    return hook_download(H, Out_inout, dO, (size_t)n * ldo * sizeof(float));
}

// randn: X[:, :b] = the solvers' starting block for `seed`
extern "C" int gemhip_test_hope_randn(int64_t n, int32_t b, int32_t ld, uint64_t seed, float *X_inout)
{
    GEMHIP_REQUIRE(n >= 1 && b >= 1 && ld >= b && X_inout, "test_hope_randn: bad arguments");
    Hope H; H.n = n;
    DevBuf<float> dX;
    HOPE_TRY(H, dX.upload(X_inout, (size_t)n * ld));
    randn(H, dX, b, ld, seed);
    return hook_download(H, X_inout, dX, (size_t)n * ld * sizeof(float));
}
