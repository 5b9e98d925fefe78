// hope_ops.hip -- the kernels of HOPE (Katz-proximity truncated SVD), Laplacian Eigenmaps and LLE for MI355X (gfx950), and one launch function
// per operation (interface: hope_ops.hpp).  The solvers that call them are in hope_solve.hip, the entry points in hope.hip.
//
// HOPE replaces gem/embedding/hope.py:28-36:
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
#include "hope_ops.hpp"
#include "sym_eig.hpp"
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

}  // namespace

namespace gemhip {

// ---------------------------------------------------------------------- solver state
void refresh_knobs(Hope &H) { H.knobs = hope_knobs_from_env([](const char *name) -> const char * { return getenv(name); }); }

Hope::Hope() { refresh_knobs(*this); }

// ---------------------------------------------------------------------- launch functions
// Y[:, :b] = alpha Op X + wa Wadd + wb W2 over the H.n rows; Op = the CSR matrix in H, or its transpose.  H.knobs.spmm16 / spmm16_u pick the kernel.
void spmm(Hope &H, bool transpose, float alpha, const float *X, int ldx, const float *Wadd, int ldw, float *Y, int ldy, int b,
          float wa, const float *W2, int ldw2, float wb)
{
    if (H.err) return;
    const int64_t blocks = (H.n + 3) / 4;
    const dim3 grid((unsigned)((blocks + NUM_XCD - 1) / NUM_XCD * NUM_XCD)), blk(256);
    const int64_t *rp = transpose ? H.rpT : H.rp; const int32_t *ci = transpose ? H.ciT : H.ci; const float *va = transpose ? H.vaT : H.va;
    if (H.knobs.spmm16 && b <= 128) {
        const int64_t blocks16 = (H.n + 15) / 16;
        const dim3 grid16((unsigned)((blocks16 + NUM_XCD - 1) / NUM_XCD * NUM_XCD));
        const int c16 = (b + 15) / 16;
#define SPMM16(C, U) do { H.last_spmm_c = C; H.last_spmm_u = U; hipLaunchKernelGGL((hope_spmm16_kernel<C, U>), grid16, blk, 0, H.s, H.n, rp, ci, va, alpha, X, ldx, Wadd, ldw, Y, ldy, b, wa, W2, ldw2, wb); } while (0)
        // gathers in flight per row and round (GEMHIP_HOPE_SPMM16_U overrides): with a row's (column, value) pairs already in the group's registers the
        // rounds are separated by arithmetic only, and the bound is registers: U x ceil(b / 16) values per lane -- 8 up to 48 columns, 4 up to 80, 2 beyond
        // (round 5: 4.21 -> 3.92 ms of SpMM per eigen-path solve at SBM 100k/1M against round 4's U = 4 with a per-round pair prefetch)
        const int uu = H.knobs.spmm16_u > 0 ? H.knobs.spmm16_u : (c16 <= 3 ? 8 : 4);
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
void gram_launch(Hope &H, const float *X, int ldx, int m1, const float *Y, int ldy, int m2, float *Gf, bool second)
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
    if (!H.knobs.colmax2) { hipLaunchKernelGGL(hope_colmax_kernel, dim3(mc), dim3(256), 0, H.s, H.n, X, ld, val); return; }
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

// after the stream has been synchronised: total time between the recorded (start, stop) pairs
void spmm_time_collect(Hope &H)
{
    for (size_t i = 0; i + 1 < H.sp_used; i += 2) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, H.sp_pool[i], H.sp_pool[i + 1]) == hipSuccess) H.spmm_ms += ms;
    }
    H.sp_used = 0;
}

// ---------------------------------------------------------------------- operator applications
// Z = S X (X: n x b):  W0 = beta A X ; Z <- W0 + beta A Z, `terms` times  => sum_{t=1..terms+1} (beta A)^t X.
// W0, T0, T1: scratch n x b with leading dimension ldt.
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

// ---------------------------------------------------------------------- set-up and statistics
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

void reset_solve_stats(Hope &H) { H.err = 0; H.spmm_count = 0; H.spmm_cols = 0; H.spmm_ms = 0; H.sp_used = 0; reset_eig_stats(); }

}  // namespace gemhip
