// tsne.hip -- t-SNE of an embedding to two dimensions (gemhip_tsne_*), the step of upstream GEM's example flow that plots an embedding:
// gem/evaluation/visualize_embedding.py:9-12 sends d > 2 through sklearn.manifold.TSNE(n_components=2).  DESIGN.md 3.5.2.
//
// Set-up (gemhip_tsne_create), every phase its own kernel launch on the null stream:
//   tsne_colsum_kernel / tsne_mean_kernel / tsne_center_kernel   column means (fp64, slabs reduced in slab order); rows minus the mean, zero-padded
//                                                                to a multiple of 8 columns, and their squared norms
//   tsne_knn_kernel          32 rows x 128 columns of ||a||^2 + ||b||^2 - 2 a.b per workgroup step on the fp32 matrix units, a running list of
//                            the k smallest (distance, id) keys per row -- no n x n matrix
//   tsne_knn_finish_kernel   the kept ids' distances again as sum_c (x_ic - x_jc)^2, rows sorted ascending by (distance, id)
//   tsne_affinity_kernel     one wavefront per row: sklearn's _binary_search_perplexity in fp64
//   tsne_count / tsne_scan / tsne_fill / tsne_sort_rows / tsne_pair   the transpose of the kNN graph as a CSR whose rows are sorted by source
//                            id, and for every arc i -> j whether (and with what p) j -> i exists
// One iteration (gemhip_tsne_run):
//   tsne_repulse_kernel      exact sum_j w^2 (y_i - y_j) and sum_j w, w = 1 / (1 + |y_i - y_j|^2): rows in registers, tiles of y_j in LDS read as
//                            broadcasts, j split across the grid in slices
//   tsne_reduce_rep_kernel   the slices' partials in slice order (fp64);  block_sum_f64_kernel (eval_common.hpp): Z = sum of the rows' sums, one workgroup, fixed order
//   tsne_attract_kernel      one wavefront per row: the sparse sums over the row's own list and over the transposed arcs that are not mutual,
//                            KL over the same nonzeros, grad = 4 (exaggeration * attr - rep / Z)
//   tsne_update_kernel       sklearn's _gradient_descent step (gains, momentum)
//
// Why the result is the same bits on every run: the only atomics are integer counters (tsne_count, tsne_fill), and what tsne_fill leaves in an
// order that depends on scheduling, tsne_sort_rows sorts by a key that is unique inside a row.  Every floating-point sum has a fixed shape: a
// thread's own elements in index order, then a butterfly over the wavefront (a + b == b + a, so every lane holds the same bits), slices and
// slabs in index order.  The k smallest keys of a row are a set: the order in which tsne_knn_kernel meets the candidates does not change it.
#include "eval_common.hpp"
#include <cmath>
#include <memory>

using namespace gemhip;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int K_MAX = 301;                            // floor(3 * 100) + 1
constexpr int AFF_PER_LANE = 5;                       // tsne_affinity_kernel: a row's distances live in registers, 5 per lane
constexpr int AFF_K_MAX = AFF_PER_LANE * WAVE;        // 320
constexpr int KNN_ROWS = 32, KNN_COLS = 128;          // one workgroup step: 4 wavefronts, one 32 x 32 MFMA tile each
constexpr int KNN_BLOCK = 256, KNN_TP = KNN_COLS + 1; // LDS row pitch of the distance tile
constexpr int REP_BLOCK = 256, REP_R = 2;             // tsne_repulse_kernel: threads per workgroup, rows per thread
constexpr int REP_ROWS = REP_BLOCK * REP_R;           // 512 rows per workgroup
constexpr int REP_TJ = 256;                           // y_j per LDS tile
constexpr int REP_CHUNK = 64;                         // consecutive y_j summed in fp32 before the sums go to fp64
constexpr int REP_TARGET_GRID = 1024;                 // workgroups wanted: four per CU
constexpr int SUM_BLOCK = 1024;
constexpr double MACHINE_EPS = 2.220446049250313e-16; // np.finfo(np.double).eps, the clamp of sklearn's _kl_divergence

// ================================================================== centring
// part[s][c] = sum over the rows of slab s of X[.][c]
__global__ __launch_bounds__(256) void tsne_colsum_kernel(const float *__restrict__ X, int64_t n, int d, int64_t ld, int64_t rows_per_slab,
                                                          double *__restrict__ part)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
    const int64_t r1 = r0 + rows_per_slab < n ? r0 + rows_per_slab : n;
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) s += (double)X[r * ld + c];
    part[(int64_t)blockIdx.y * d + c] = s;
}

__global__ __launch_bounds__(256) void tsne_mean_kernel(const double *__restrict__ part, int nslabs, int d, int64_t n, float *__restrict__ mean)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double s = 0.0;
    for (int k = 0; k < nslabs; ++k) s += part[(int64_t)k * d + c];
    mean[c] = (float)(s / (double)n);
}

// Xc[i][0 .. dpad) = X[i][c] - mean[c], zero from d on; norm[i] = |Xc[i]|^2.  One wavefront per row.
__global__ __launch_bounds__(256) void tsne_center_kernel(const float *__restrict__ X, int64_t n, int d, int64_t ld, const float *__restrict__ mean, int dpad,
                                                          float *__restrict__ Xc, float *__restrict__ norm)
{
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    float s = 0.f;
    for (int c = lane; c < dpad; c += WAVE) {
        const float v = c < d ? X[i * ld + c] - mean[c] : 0.f;
        Xc[i * dpad + c] = v;
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) norm[i] = s;
}

// ================================================================== kNN
// A row's list: k keys (distance bits << 32 | id) in no particular order; position t is only ever written and read by lane t % 64 of the one
// wavefront that owns the row, so the list needs no ordering between lanes.  While it is filling, keys are appended; once full, a key smaller
// than the list's maximum replaces it and the maximum is found again.
__device__ __forceinline__ void knn_insert(u64 *__restrict__ L, int k, u64 key, u64 &thr, int &cnt, int &maxpos, int lane)
{
    const int pos = cnt < k ? cnt : maxpos;
    if ((pos & (WAVE - 1)) == lane) L[pos] = key;
    if (cnt < k) {
        ++cnt;
        if (cnt < k) return;
    }
    u64 best = 0;
    int bpos = -1;
    for (int t = lane; t < k; t += WAVE) {
        const u64 v = t == pos ? key : L[t];
        if (bpos < 0 || v > best) { best = v; bpos = t; }
    }
    u64 top = best;
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(top, off);
        top = o > top ? o : top;
    }
    const u64 who = __ballot(bpos >= 0 && best == top);          // keys are unique (the id is part of them): exactly one lane
    maxpos = __shfl(bpos, __ffsll(who) - 1);
    thr = top;
}

// Workgroup b owns rows [32 b, 32 b + 32); wavefront w computes columns [128 t + 32 w, +32) of step t and afterwards scans rows 8 w .. 8 w + 7
// of the step's 32 x 128 distances.  MFMA 32x32x2: lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31]; which two of the dpad products
// the two lane halves supply per instruction is free as long as A and B agree, so half h walks columns [h dpad/2, (h + 1) dpad/2) of its row
// with 16-byte loads.  keys: [n][k], scratch.
__global__ __launch_bounds__(KNN_BLOCK) void tsne_knn_kernel(const float *__restrict__ Xc, const float *__restrict__ norm, int64_t n, int dpad, int k,
                                                             u64 *__restrict__ keys)
{
    __shared__ float tile[KNN_ROWS][KNN_TP];
    __shared__ float na_s[KNN_ROWS];
    const int lane = lane_id(), wave = threadIdx.x >> 6, h = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * KNN_ROWS;
    const int half = dpad >> 1, nq = half >> 2;
    const int64_t arow = row0 + l31 < n ? row0 + l31 : n - 1;
    const f32x4 *pa = reinterpret_cast<const f32x4 *>(Xc + arow * dpad + h * half);
    if (threadIdx.x < KNN_ROWS) na_s[threadIdx.x] = norm[row0 + threadIdx.x < n ? row0 + threadIdx.x : n - 1];
    u64 thr[8];
    int cnt[8], maxpos[8];
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) { thr[rr] = ~0ull; cnt[rr] = 0; maxpos[rr] = 0; }
    __syncthreads();
    for (int64_t c0 = 0; c0 < n; c0 += KNN_COLS) {
        const int64_t col = c0 + wave * 32 + l31;
        const int64_t bcol = col < n ? col : n - 1;
        const f32x4 *pb = reinterpret_cast<const f32x4 *>(Xc + bcol * dpad + h * half);
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        for (int t = 0; t < nq; ++t) {
            const f32x4 a = pa[t], b = pb[t];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
        }
        const float nb = norm[bcol];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int r = (q & 3) + 8 * (q >> 2) + 4 * h;                     // C/D map of the 32x32 MFMA
            tile[r][wave * 32 + l31] = fmaxf(fmaf(-2.f, acc[q], na_s[r] + nb), 0.f);
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 8; ++rr) {
            const int r = wave * 8 + rr;
            const int64_t gi = row0 + r;
            if (gi >= n) continue;                                            // (the same in all lanes)
            u64 *L = keys + gi * k;
#pragma unroll
            for (int part = 0; part < KNN_COLS / WAVE; ++part) {
                const int cc = lane + WAVE * part;
                const int64_t cj = c0 + cc;
                const u64 key = ((u64)__float_as_uint(tile[r][cc]) << 32) | (u64)(uint32_t)cj;
                u64 todo = __ballot(cj < n && cj != gi && key < thr[rr]);
                while (todo) {                                                // (the same in all lanes)
                    const int from = __ffsll(todo) - 1;
                    todo &= todo - 1;
                    const u64 cand = __shfl(key, from);
                    if (cand < thr[rr]) knn_insert(L, k, cand, thr[rr], cnt[rr], maxpos[rr], lane);
                }
            }
        }
        __syncthreads();                                                      // the next step overwrites the tile
    }
}

// One wavefront per row: the kept ids' distances from the rows themselves, then a rank sort by (distance, id) through LDS.
__global__ __launch_bounds__(256) void tsne_knn_finish_kernel(const float *__restrict__ X, int64_t n, int d, int64_t ld, int k, const u64 *__restrict__ keys,
                                                              int32_t *__restrict__ id_out, float *__restrict__ dist_out)
{
    __shared__ u64 sk[4][K_MAX + 3];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    const bool live = i < n;
    if (live) {
        const float *xi = X + i * ld;
        for (int t = lane; t < k; t += WAVE) {
            const uint32_t j = (uint32_t)(keys[i * k + t] & 0xFFFFFFFFull);
            const float *xj = X + (int64_t)j * ld;
            float s = 0.f;
            for (int c = 0; c < d; ++c) {
                const float df = xi[c] - xj[c];
                s = fmaf(df, df, s);
            }
            sk[wave][t] = ((u64)__float_as_uint(s) << 32) | (u64)j;
        }
    }
    __syncthreads();
    if (!live) return;
    for (int t = lane; t < k; t += WAVE) {
        const u64 mine = sk[wave][t];
        int rank = 0;
        for (int u = 0; u < k; ++u) rank += sk[wave][u] < mine ? 1 : 0;
        id_out[i * k + rank] = (int32_t)(uint32_t)(mine & 0xFFFFFFFFull);
        dist_out[i * k + rank] = __uint_as_float((uint32_t)(mine >> 32));
    }
}

// ================================================================== conditional affinities
// sklearn/manifold/_utils.pyx _binary_search_perplexity restated: the distances are float32, everything else double; the result is rounded to
// float32 once.  One wavefront per row.
__global__ __launch_bounds__(256) void tsne_affinity_kernel(const float *__restrict__ dist, int64_t n, int k, double perplexity, float *__restrict__ p_out)
{
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    double dv[AFF_PER_LANE], pv[AFF_PER_LANE];
#pragma unroll
    for (int m = 0; m < AFF_PER_LANE; ++m) {
        const int t = lane + WAVE * m;
        dv[m] = t < k ? (double)dist[i * k + t] : 0.0;
        pv[m] = 0.0;
    }
    const double desired = log(perplexity);
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    for (int step = 0; step < 100; ++step) {
        double sum_p = 0.0;
#pragma unroll
        for (int m = 0; m < AFF_PER_LANE; ++m)
            if (lane + WAVE * m < k) {
                pv[m] = exp(-dv[m] * beta);
                sum_p += pv[m];
            }
        sum_p = wave_sum_f64(sum_p);
        if (sum_p == 0.0) sum_p = 1e-8;
        double sum_dp = 0.0;
#pragma unroll
        for (int m = 0; m < AFF_PER_LANE; ++m)
            if (lane + WAVE * m < k) {
                pv[m] = pv[m] / sum_p;
                sum_dp += dv[m] * pv[m];
            }
        sum_dp = wave_sum_f64(sum_dp);
        const double diff = log(sum_p) + beta * sum_dp - desired;
        if (fabs(diff) <= 1e-5) break;
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
#pragma unroll
    for (int m = 0; m < AFF_PER_LANE; ++m)
        if (lane + WAVE * m < k) p_out[i * k + lane + WAVE * m] = (float)pv[m];
}

// ================================================================== transpose of the kNN graph
__global__ __launch_bounds__(256) void tsne_count_kernel(const int32_t *__restrict__ id, int64_t total, int32_t *count)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) atomicAdd(count + id[e], 1);
}

// ptr[0 .. n] = exclusive prefix of count[0 .. n).  ONE workgroup, SUM_BLOCK counts per pass with a running carry.
__global__ __launch_bounds__(SUM_BLOCK) void tsne_scan_kernel(const int32_t *__restrict__ count, int64_t n, int32_t *__restrict__ ptr)
{
    __shared__ int32_t wave_total[SUM_BLOCK / WAVE];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    int32_t carry = 0;
    for (int64_t base = 0; base < n; base += SUM_BLOCK) {
        const int64_t t = base + threadIdx.x;
        const int32_t c = t < n ? count[t] : 0;
        int32_t incl = c;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int32_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (lane == WAVE - 1) wave_total[wave] = incl;
        __syncthreads();
        int32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < SUM_BLOCK / WAVE; ++w) {
            const int32_t s = wave_total[w];
            before += w < wave ? s : 0;
            all += s;
        }
        __syncthreads();
        if (t < n) ptr[t] = carry + before + incl - c;
        carry += all;
    }
    if (threadIdx.x == 0) ptr[n] = carry;
}

// Arc e = (i -> id[e]) goes to some free slot of row id[e]: WHICH slot depends on scheduling, tsne_sort_rows_kernel undoes that.
__global__ __launch_bounds__(256) void tsne_fill_kernel(const int32_t *__restrict__ id, const float *__restrict__ p, int64_t total, int k,
                                                        const int32_t *__restrict__ ptr, int32_t *cursor, int32_t *__restrict__ src_tmp, float *__restrict__ p_tmp)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int32_t j = id[e];
    const int32_t slot = ptr[j] + atomicAdd(cursor + j, 1);
    src_tmp[slot] = (int32_t)(e / k);
    p_tmp[slot] = p[e];
}

// One wavefront per row: rank sort by source id (a source occurs once in a row: ranks are a permutation).
__global__ __launch_bounds__(256) void tsne_sort_rows_kernel(int64_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ src_tmp,
                                                             const float *__restrict__ p_tmp, int32_t *__restrict__ t_src, float *__restrict__ t_p)
{
    const int lane = lane_id();
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const int32_t b = ptr[j], len = ptr[j + 1] - b;
    for (int32_t t = lane; t < len; t += WAVE) {
        const int32_t s = src_tmp[b + t];
        int32_t rank = 0;
        for (int32_t u = 0; u < len; ++u) rank += src_tmp[b + u] < s ? 1 : 0;
        t_src[b + rank] = s;
        t_p[b + rank] = p_tmp[b + t];
    }
}

// For arc e = (i -> j): is j -> i an arc too?  Row i of the transpose holds the sources s of the arcs s -> i with p_{i|s}: look j up there.
// f_pt[e] = p_{i|j} or 0; the transposed entry found is marked mutual (one writer: the pair (i, j) occurs once).
__global__ __launch_bounds__(256) void tsne_pair_kernel(const int32_t *__restrict__ id, int64_t total, int k, const int32_t *__restrict__ ptr,
                                                        const int32_t *__restrict__ t_src, const float *__restrict__ t_p, float *__restrict__ f_pt,
                                                        uint8_t *__restrict__ t_mut)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t i = e / k;
    const int32_t j = id[e];
    int32_t lo = ptr[i], hi = ptr[i + 1];
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo) / 2;
        if (t_src[mid] < j) lo = mid + 1; else hi = mid;
    }
    float back = 0.f;
    if (lo < ptr[i + 1] && t_src[lo] == j) {
        back = t_p[lo];
        t_mut[lo] = 1;
    }
    f_pt[e] = back;
}

// ================================================================== gradient
// part[(s * 3 + c) * n + i], c = 0, 1: sum over slice s of w^2 (y_i - y_j); c = 2: sum of w (the pair j == i included: exactly 1.0).
// fp32 inside a chunk of REP_CHUNK columns, fp64 from chunk to chunk.
__global__ __launch_bounds__(REP_BLOCK) void tsne_repulse_kernel(const float2 *__restrict__ Y, int64_t n, int64_t jslice, double *__restrict__ part)
{
    __shared__ float2 ty[REP_TJ];
    const int64_t i0 = (int64_t)blockIdx.x * REP_ROWS + threadIdx.x;
    float2 yi[REP_R];
    double fx[REP_R], fy[REP_R], fz[REP_R];
#pragma unroll
    for (int r = 0; r < REP_R; ++r) {
        const int64_t i = i0 + (int64_t)r * REP_BLOCK;
        yi[r] = Y[i < n ? i : n - 1];
        fx[r] = fy[r] = fz[r] = 0.0;
    }
    const int64_t j_begin = (int64_t)blockIdx.y * jslice;
    const int64_t j_end = j_begin + jslice < n ? j_begin + jslice : n;
    for (int64_t j0 = j_begin; j0 < j_end; j0 += REP_TJ) {
        const int jn = (int)(j_end - j0 < REP_TJ ? j_end - j0 : REP_TJ);
        __syncthreads();
        if ((int)threadIdx.x < jn) ty[threadIdx.x] = Y[j0 + threadIdx.x];
        __syncthreads();
        for (int jb = 0; jb < jn; jb += REP_CHUNK) {
            const int je = jb + REP_CHUNK < jn ? jb + REP_CHUNK : jn;
            float sx[REP_R], sy[REP_R], sz[REP_R];
#pragma unroll
            for (int r = 0; r < REP_R; ++r) sx[r] = sy[r] = sz[r] = 0.f;
#pragma unroll 8
            for (int jj = jb; jj < je; ++jj) {
                const float2 yj = ty[jj];
#pragma unroll
                for (int r = 0; r < REP_R; ++r) {
                    const float dx = yi[r].x - yj.x, dy = yi[r].y - yj.y;
                    const float w = __builtin_amdgcn_rcpf(fmaf(dx, dx, fmaf(dy, dy, 1.f)));
                    const float w2 = w * w;
                    sz[r] += w;
                    sx[r] = fmaf(w2, dx, sx[r]);
                    sy[r] = fmaf(w2, dy, sy[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < REP_R; ++r) { fx[r] += (double)sx[r]; fy[r] += (double)sy[r]; fz[r] += (double)sz[r]; }
        }
    }
#pragma unroll
    for (int r = 0; r < REP_R; ++r) {
        const int64_t i = i0 + (int64_t)r * REP_BLOCK;
        if (i < n) {
            double *o = part + (int64_t)blockIdx.y * 3 * n + i;
            o[0] = fx[r]; o[n] = fy[r]; o[2 * n] = fz[r];
        }
    }
}

// rep[i], rep[n + i] = the slices' force sums in slice order; zrow[i] = the row's sum of w without its own pair.
__global__ __launch_bounds__(256) void tsne_reduce_rep_kernel(const double *__restrict__ part, int64_t n, int nslices, double *__restrict__ rep,
                                                              double *__restrict__ zrow)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double x = 0.0, y = 0.0, z = 0.0;
    for (int s = 0; s < nslices; ++s) {
        const double *o = part + (int64_t)s * 3 * n + i;
        x += o[0]; y += o[n]; z += o[2 * n];
    }
    rep[i] = x; rep[n + i] = y; zrow[i] = z - 1.0;
}

// One nonzero P_ij of row i: attr += P w (y_i - y_j), kl += P log(max(P, eps) / max(w / Z, eps)).  fp64 (the sums are short).
__device__ __forceinline__ void attract_term(double P, float2 yi, float2 yj, double Z, bool want_kl, double &ax, double &ay, double &kl)
{
    const double dx = (double)yi.x - (double)yj.x, dy = (double)yi.y - (double)yj.y;
    const double w = 1.0 / (1.0 + dx * dx + dy * dy);
    ax += P * w * dx;
    ay += P * w * dy;
    if (want_kl) {
        const double q = w / Z;
        kl += P * log((P > MACHINE_EPS ? P : MACHINE_EPS) / (q > MACHINE_EPS ? q : MACHINE_EPS));
    }
}

// One wavefront per row.  P_ij = (p_{j|i} + p_{i|j}) / 2n over the row's own arcs (f_pt carries p_{i|j} where j -> i exists), and p_{i|j} / 2n
// over the transposed arcs that are not mutual: together every nonzero of row i of the symmetrised P once.
__global__ __launch_bounds__(256) void tsne_attract_kernel(const float2 *__restrict__ Y, int64_t n, int k, const int32_t *__restrict__ id,
                                                           const float *__restrict__ p, const float *__restrict__ f_pt, const int32_t *__restrict__ ptr,
                                                           const int32_t *__restrict__ t_src, const float *__restrict__ t_p,
                                                           const uint8_t *__restrict__ t_mut, const double *__restrict__ rep,
                                                           const double *__restrict__ zsum, double exaggeration, int want_kl,
                                                           float2 *__restrict__ grad, double *__restrict__ klrow)
{
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const double Z = *zsum, inv2n = 0.5 / (double)n;
    const float2 yi = Y[i];
    double ax = 0.0, ay = 0.0, kl = 0.0;
    for (int t = lane; t < k; t += WAVE) {
        const int64_t e = i * k + t;
        attract_term(((double)p[e] + (double)f_pt[e]) * inv2n, yi, Y[id[e]], Z, want_kl != 0, ax, ay, kl);
    }
    const int32_t b = ptr[i], len = ptr[i + 1] - b;
    for (int32_t t = lane; t < len; t += WAVE)
        if (!t_mut[b + t]) attract_term((double)t_p[b + t] * inv2n, yi, Y[t_src[b + t]], Z, want_kl != 0, ax, ay, kl);
    ax = wave_sum_f64(ax);
    ay = wave_sum_f64(ay);
    if (want_kl) kl = wave_sum_f64(kl);
    if (lane == 0) {
        grad[i] = make_float2((float)(4.0 * (exaggeration * ax - rep[i] / Z)), (float)(4.0 * (exaggeration * ay - rep[n + i] / Z)));
        if (want_kl) klrow[i] = kl;
    }
}

// sklearn/manifold/_t_sne.py _gradient_descent, one step, float32 like its arrays.
__device__ __forceinline__ void update_one(float g, float &u, float &gain, float &y, float momentum, float lr, double &gn2)
{
    gain = u * g < 0.f ? gain + 0.2f : gain * 0.8f;
    gain = gain < 0.01f ? 0.01f : gain;
    const float gg = __fmul_rn(g, gain);
    u = __fsub_rn(__fmul_rn(momentum, u), __fmul_rn(lr, gg));
    y = __fadd_rn(y, u);
    gn2 += (double)gg * (double)gg;
}

__global__ __launch_bounds__(256) void tsne_update_kernel(int64_t n, const float2 *__restrict__ grad, float2 *__restrict__ upd, float2 *__restrict__ gains,
                                                          float2 *__restrict__ Y, float momentum, float lr, double *__restrict__ gnrow)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float2 g = grad[i];
    float2 u = upd[i], ga = gains[i], y = Y[i];
    double gn2 = 0.0;
    update_one(g.x, u.x, ga.x, y.x, momentum, lr, gn2);
    update_one(g.y, u.y, ga.y, y.y, momentum, lr, gn2);
    upd[i] = u; gains[i] = ga; Y[i] = y; gnrow[i] = gn2;
}

__global__ __launch_bounds__(256) void tsne_reset_kernel(int64_t n, float2 *__restrict__ upd, float2 *__restrict__ gains)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    upd[i] = make_float2(0.f, 0.f);
    gains[i] = make_float2(1.f, 1.f);
}

// ================================================================== host side
int check_matrix(const char *who, int64_t n, int32_t d, int32_t ld, const float *X)
{
    const int rc = check_embedding(who, n, d, ld, X, 2, 0, nullptr);
    if (rc) return rc;
    const int64_t bad = first_bad_entry(X, n, d, ld, 1e15f);
    GEMHIP_REQUIRE(bad < 0, "%s: X[%lld][%d] = %g is not finite or above 1e15 in magnitude", who, (long long)(bad / d), (int)(bad % d),
                   (double)X[bad / d * ld + bad % d]);
    return GEMHIP_OK;
}

int k_of(double perplexity, int64_t n)
{
    const int64_t k = (int64_t)std::floor(3.0 * perplexity) + 1;
    return (int)(k < n - 1 ? k : n - 1);
}

// X on the device, [n][ld] -> id, dist [n][k].  Enqueues and returns; the scratch lives until the caller's buffers go (the frees synchronise).
int knn_device(const float *dX, int64_t n, int d, int64_t ld, int k, int32_t *id, float *dist)
{
    const int dpad = (d + 7) & ~7;
    const int64_t rows_per_slab = (n + 4095) / 4096 > 256 ? (n + 4095) / 4096 : 256;       // at most 4096 slabs
    const int nslabs = (int)((n + rows_per_slab - 1) / rows_per_slab);
    DevBuf<double> part;
    DevBuf<float> mean, Xc, norm;
    DevBuf<u64> keys;
    GEMHIP_CHECK(part.reserve((size_t)nslabs * d));
    GEMHIP_CHECK(mean.reserve((size_t)d));
    GEMHIP_CHECK(Xc.reserve((size_t)n * dpad));
    GEMHIP_CHECK(norm.reserve((size_t)n));
    GEMHIP_CHECK(keys.reserve((size_t)n * k));
    GEMHIP_CHECK(hipMemsetAsync(keys, 0, (size_t)n * k * sizeof(u64), 0));          // (every slot is written: n - 1 >= k finite candidates per row; a slot
                                                                                    // that were not would then name row 0, never memory outside X)
    hipLaunchKernelGGL(tsne_colsum_kernel, dim3(grid_of(d, 256), (unsigned)nslabs), dim3(256), 0, 0, dX, n, d, ld, rows_per_slab, part.get());
    hipLaunchKernelGGL(tsne_mean_kernel, dim3(grid_of(d, 256)), dim3(256), 0, 0, part.get(), nslabs, d, n, mean.get());
    hipLaunchKernelGGL(tsne_center_kernel, dim3(grid_of(n, 4)), dim3(256), 0, 0, dX, n, d, ld, mean.get(), dpad, Xc.get(), norm.get());
    hipLaunchKernelGGL(tsne_knn_kernel, dim3(grid_of(n, KNN_ROWS)), dim3(KNN_BLOCK), 0, 0, Xc.get(), norm.get(), n, dpad, k, keys.get());
    hipLaunchKernelGGL(tsne_knn_finish_kernel, dim3(grid_of(n, 4)), dim3(256), 0, 0, dX, n, d, ld, k, keys.get(), id, dist);
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipDeviceSynchronize());
    return GEMHIP_OK;
}

}  // namespace

struct gemhip_tsne {
    int64_t n = 0;
    int d = 0, k = 0, nslices = 1;
    int64_t jslice = 0;
    double perplexity = 0.0;
    bool have_y = false;
    DevBuf<int32_t> id, t_ptr, t_src;
    DevBuf<float> p, f_pt, t_p;
    DevBuf<uint8_t> t_mut;
    DevBuf<float2> Y, upd, gains, grad;
    DevBuf<double> part, rep, zrow, klrow, gnrow, scal;          // scal: {Z, KL, |gains * grad|^2}
    Stopwatch watch;
    double ms[4] = {0, 0, 0, 0};
};

namespace {

// From h->id and h->p: the transpose (t_ptr, t_src, t_p), f_pt and t_mut.
int build_transpose(gemhip_tsne *h)
{
    const int64_t n = h->n, total = n * h->k;
    DevBuf<int32_t> count, cursor, src_tmp;
    DevBuf<float> p_tmp;
    GEMHIP_CHECK(count.reserve((size_t)n));
    GEMHIP_CHECK(cursor.reserve((size_t)n));
    GEMHIP_CHECK(src_tmp.reserve((size_t)total));
    GEMHIP_CHECK(p_tmp.reserve((size_t)total));
    GEMHIP_CHECK(h->t_ptr.reserve((size_t)n + 1));
    GEMHIP_CHECK(h->t_src.reserve((size_t)total));
    GEMHIP_CHECK(h->t_p.reserve((size_t)total));
    GEMHIP_CHECK(h->f_pt.reserve((size_t)total));
    GEMHIP_CHECK(h->t_mut.reserve((size_t)total));
    GEMHIP_CHECK(hipMemsetAsync(count, 0, (size_t)n * sizeof(int32_t), 0));
    GEMHIP_CHECK(hipMemsetAsync(cursor, 0, (size_t)n * sizeof(int32_t), 0));
    GEMHIP_CHECK(hipMemsetAsync(h->t_mut, 0, (size_t)total, 0));
    const unsigned ge = grid_of(total, 256);
    hipLaunchKernelGGL(tsne_count_kernel, dim3(ge), dim3(256), 0, 0, h->id.get(), total, count.get());
    hipLaunchKernelGGL(tsne_scan_kernel, dim3(1), dim3(SUM_BLOCK), 0, 0, count.get(), n, h->t_ptr.get());
    hipLaunchKernelGGL(tsne_fill_kernel, dim3(ge), dim3(256), 0, 0, h->id.get(), h->p.get(), total, h->k, h->t_ptr.get(), cursor.get(), src_tmp.get(), p_tmp.get());
    hipLaunchKernelGGL(tsne_sort_rows_kernel, dim3(grid_of(n, 4)), dim3(256), 0, 0, n, h->t_ptr.get(), src_tmp.get(), p_tmp.get(), h->t_src.get(), h->t_p.get());
    hipLaunchKernelGGL(tsne_pair_kernel, dim3(ge), dim3(256), 0, 0, h->id.get(), total, h->k, h->t_ptr.get(), h->t_src.get(), h->t_p.get(), h->f_pt.get(), h->t_mut.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipDeviceSynchronize());
    return GEMHIP_OK;
}

// Enqueue one gradient at h->Y: grad, and with want_kl scal[1] = KL.  scal[0] = Z always.
int enqueue_gradient(gemhip_tsne *h, double exaggeration, bool want_kl)
{
    const int64_t n = h->n;
    hipLaunchKernelGGL(tsne_repulse_kernel, dim3(grid_of(n, REP_ROWS), (unsigned)h->nslices), dim3(REP_BLOCK), 0, 0, h->Y.get(), n, h->jslice, h->part.get());
    hipLaunchKernelGGL(tsne_reduce_rep_kernel, dim3(grid_of(n, 256)), dim3(256), 0, 0, h->part.get(), n, h->nslices, h->rep.get(), h->zrow.get());
    hipLaunchKernelGGL((block_sum_f64_kernel<SUM_BLOCK, gemhip_tsne>), dim3(1), dim3(SUM_BLOCK), 0, 0, h->zrow.get(), n, h->scal.get());
    hipLaunchKernelGGL(tsne_attract_kernel, dim3(grid_of(n, 4)), dim3(256), 0, 0, h->Y.get(), n, h->k, h->id.get(), h->p.get(), h->f_pt.get(), h->t_ptr.get(),
                       h->t_src.get(), h->t_p.get(), h->t_mut.get(), h->rep.get(), h->scal.get(), exaggeration, want_kl ? 1 : 0, h->grad.get(), h->klrow.get());
    if (want_kl) hipLaunchKernelGGL((block_sum_f64_kernel<SUM_BLOCK, gemhip_tsne>), dim3(1), dim3(SUM_BLOCK), 0, 0, h->klrow.get(), n, h->scal.get() + 1);
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

int alloc_iteration_state(gemhip_tsne *h)
{
    const int64_t n = h->n;
    const int64_t rowblocks = (n + REP_ROWS - 1) / REP_ROWS, tiles = (n + REP_TJ - 1) / REP_TJ;
    int64_t want = (REP_TARGET_GRID + rowblocks - 1) / rowblocks;
    want = want < 1 ? 1 : want > tiles ? tiles : want;
    h->jslice = (tiles + want - 1) / want * REP_TJ;
    h->nslices = (int)((n + h->jslice - 1) / h->jslice);
    GEMHIP_CHECK(h->Y.reserve((size_t)n));
    GEMHIP_CHECK(h->upd.reserve((size_t)n));
    GEMHIP_CHECK(h->gains.reserve((size_t)n));
    GEMHIP_CHECK(h->grad.reserve((size_t)n));
    GEMHIP_CHECK(h->part.reserve((size_t)h->nslices * 3 * n));
    GEMHIP_CHECK(h->rep.reserve((size_t)2 * n));
    GEMHIP_CHECK(h->zrow.reserve((size_t)n));
    GEMHIP_CHECK(h->klrow.reserve((size_t)n));
    GEMHIP_CHECK(h->gnrow.reserve((size_t)n));
    GEMHIP_CHECK(h->scal.reserve(4));
    return GEMHIP_OK;
}

}  // namespace

extern "C" int gemhip_tsne_create(int64_t n, int32_t d, int32_t ld, const float *X_host, double perplexity, gemhip_tsne_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "tsne_create: NULL output");
    *out = nullptr;
    GEMHIP_REQUIRE(perplexity >= 5.0 && perplexity <= 100.0, "tsne_create: perplexity = %g outside [5, 100]", perplexity);
    GEMHIP_REQUIRE((double)n > perplexity, "tsne_create: perplexity = %g must be less than n = %lld", perplexity, (long long)n);
    int rc = check_matrix("tsne_create", n, d, ld, X_host);
    if (rc) return rc;
    const int k = k_of(perplexity, n);
    if (n * k > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "tsne_create: n * k = %lld * %d: must be below 2^31", (long long)n, k);
    std::unique_ptr<gemhip_tsne> h(new gemhip_tsne);
    h->n = n; h->d = d; h->k = k; h->perplexity = perplexity;
    DevBuf<float> dX, dist;
    GEMHIP_CHECK(dX.upload(X_host, (size_t)n * ld));
    GEMHIP_CHECK(h->id.reserve((size_t)n * k));
    GEMHIP_CHECK(h->p.reserve((size_t)n * k));
    GEMHIP_CHECK(dist.reserve((size_t)n * k));
    GEMHIP_CHECK(start(h->watch));
    rc = knn_device(dX, n, d, ld, k, h->id, dist);
    if (rc) return rc;
    GEMHIP_CHECK(stop(h->watch, &h->ms[0]));
    dX.reset();
    GEMHIP_CHECK(start(h->watch));
    hipLaunchKernelGGL(tsne_affinity_kernel, dim3(grid_of(n, 4)), dim3(256), 0, 0, dist.get(), n, k, perplexity, h->p.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(stop(h->watch, &h->ms[1]));
    GEMHIP_CHECK(start(h->watch));
    rc = build_transpose(h.get());
    if (rc) return rc;
    GEMHIP_CHECK(stop(h->watch, &h->ms[2]));
    rc = alloc_iteration_state(h.get());
    if (rc) return rc;
    *out = h.release();
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_destroy(gemhip_tsne_t h)
{
    delete h;
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_info(gemhip_tsne_t h, int64_t *out)
{
    GEMHIP_REQUIRE(h && out, "tsne_info: NULL");
    out[0] = h->n; out[1] = h->d; out[2] = h->k; out[3] = h->nslices;
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_last_ms(gemhip_tsne_t h, double *out)
{
    GEMHIP_REQUIRE(h && out, "tsne_last_ms: NULL");
    for (int q = 0; q < 4; ++q) out[q] = h->ms[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_set_embedding(gemhip_tsne_t h, const float *Y_host)
{
    GEMHIP_REQUIRE(h && Y_host, "tsne_set_embedding: NULL");
    for (int64_t q = 0; q < 2 * h->n; ++q) GEMHIP_REQUIRE(std::isfinite(Y_host[q]), "tsne_set_embedding: Y[%lld][%d] is not finite", (long long)(q / 2), (int)(q % 2));
    GEMHIP_CHECK(hipMemcpy(h->Y, Y_host, (size_t)h->n * sizeof(float2), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(tsne_reset_kernel, dim3(grid_of(h->n, 256)), dim3(256), 0, 0, h->n, h->upd.get(), h->gains.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->have_y = true;
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_get_embedding(gemhip_tsne_t h, float *Y_out)
{
    GEMHIP_REQUIRE(h && Y_out, "tsne_get_embedding: NULL");
    GEMHIP_REQUIRE(h->have_y, "tsne_get_embedding: no embedding set");
    GEMHIP_CHECK(hipMemcpy(Y_out, h->Y, (size_t)h->n * sizeof(float2), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_run(gemhip_tsne_t h, int32_t n_iter, double exaggeration, double momentum, double lr, double *kl_out, double *grad_norm_out)
{
    GEMHIP_REQUIRE(h != nullptr, "tsne_run: NULL handle");
    GEMHIP_REQUIRE(h->have_y, "tsne_run: no embedding set (gemhip_tsne_set_embedding)");
    GEMHIP_REQUIRE(n_iter >= 1, "tsne_run: n_iter = %d (need >= 1)", n_iter);
    GEMHIP_REQUIRE(std::isfinite(exaggeration) && exaggeration > 0.0 && std::isfinite(momentum) && std::isfinite(lr),
                   "tsne_run: exaggeration = %g, momentum = %g, lr = %g", exaggeration, momentum, lr);
    const int64_t n = h->n;
    GEMHIP_CHECK(start(h->watch));
    for (int32_t it = 0; it < n_iter; ++it) {
        const bool last = it == n_iter - 1;
        const int rc = enqueue_gradient(h, exaggeration, last);
        if (rc) return rc;
        hipLaunchKernelGGL(tsne_update_kernel, dim3(grid_of(n, 256)), dim3(256), 0, 0, n, h->grad.get(), h->upd.get(), h->gains.get(), h->Y.get(), (float)momentum,
                           (float)lr, h->gnrow.get());
    }
    hipLaunchKernelGGL((block_sum_f64_kernel<SUM_BLOCK, gemhip_tsne>), dim3(1), dim3(SUM_BLOCK), 0, 0, h->gnrow.get(), n, h->scal.get() + 2);
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(stop(h->watch, &h->ms[3]));
    double s[3];
    GEMHIP_CHECK(hipMemcpy(s, h->scal, sizeof s, hipMemcpyDeviceToHost));
    if (kl_out) *kl_out = s[1];
    if (grad_norm_out) *grad_norm_out = std::sqrt(s[2]);
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_gradient(gemhip_tsne_t h, double exaggeration, float *grad_out, double *kl_out, double *z_out)
{
    GEMHIP_REQUIRE(h && grad_out, "tsne_gradient: NULL");
    GEMHIP_REQUIRE(h->have_y, "tsne_gradient: no embedding set (gemhip_tsne_set_embedding)");
    GEMHIP_REQUIRE(std::isfinite(exaggeration) && exaggeration > 0.0, "tsne_gradient: exaggeration = %g", exaggeration);
    const int rc = enqueue_gradient(h, exaggeration, true);
    if (rc) return rc;
    GEMHIP_CHECK(hipDeviceSynchronize());
    double s[2];
    GEMHIP_CHECK(hipMemcpy(s, h->scal, sizeof s, hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(grad_out, h->grad, (size_t)h->n * sizeof(float2), hipMemcpyDeviceToHost));
    if (z_out) *z_out = s[0];
    if (kl_out) *kl_out = s[1];
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_set_affinities(gemhip_tsne_t h, const int32_t *id, const float *p)
{
    GEMHIP_REQUIRE(h && id && p, "tsne_set_affinities: NULL");
    const int64_t n = h->n, total = n * h->k;
    for (int64_t e = 0; e < total; ++e) {
        GEMHIP_REQUIRE(id[e] >= 0 && id[e] < n && id[e] != e / h->k, "tsne_set_affinities: id[%lld][%lld] = %d outside [0,%lld) or the row itself", (long long)(e / h->k),
                       (long long)(e % h->k), id[e], (long long)n);
        GEMHIP_REQUIRE(std::isfinite(p[e]) && p[e] >= 0.f, "tsne_set_affinities: p[%lld][%lld] = %g", (long long)(e / h->k), (long long)(e % h->k), (double)p[e]);
    }
    GEMHIP_CHECK(hipMemcpy(h->id, id, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice));
    GEMHIP_CHECK(hipMemcpy(h->p, p, (size_t)total * sizeof(float), hipMemcpyHostToDevice));
    return build_transpose(h);
}

extern "C" int gemhip_tsne_knn(int64_t n, int32_t d, int32_t ld, const float *X_host, int32_t k, int32_t *id_out, float *dist_out)
{
    GEMHIP_REQUIRE(id_out && dist_out, "tsne_knn: NULL output");
    int rc = check_matrix("tsne_knn", n, d, ld, X_host);
    if (rc) return rc;
    GEMHIP_REQUIRE(k >= 1 && k <= K_MAX && k <= n - 1, "tsne_knn: k = %d (need 1 <= k <= min(n - 1, %d))", k, K_MAX);
    if (n * k > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "tsne_knn: n * k = %lld * %d: must be below 2^31", (long long)n, k);
    DevBuf<float> dX, dist;
    DevBuf<int32_t> id;
    GEMHIP_CHECK(dX.upload(X_host, (size_t)n * ld));
    GEMHIP_CHECK(id.reserve((size_t)n * k));
    GEMHIP_CHECK(dist.reserve((size_t)n * k));
    rc = knn_device(dX, n, d, ld, k, id, dist);
    if (rc) return rc;
    GEMHIP_CHECK(hipMemcpy(id_out, id, (size_t)n * k * sizeof(int32_t), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(dist_out, dist, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_tsne_affinities(int64_t n, int32_t k, const float *dist, double perplexity, float *p_out)
{
    GEMHIP_REQUIRE(dist && p_out, "tsne_affinities: NULL");
    GEMHIP_REQUIRE(n >= 1 && k >= 1 && k <= AFF_K_MAX, "tsne_affinities: n = %lld, k = %d (need n >= 1, 1 <= k <= %d)", (long long)n, k, AFF_K_MAX);
    GEMHIP_REQUIRE(perplexity >= 5.0 && perplexity <= 100.0, "tsne_affinities: perplexity = %g outside [5, 100]", perplexity);
    if (n * k > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "tsne_affinities: n * k = %lld * %d: must be below 2^31", (long long)n, k);
    for (int64_t e = 0; e < n * k; ++e) GEMHIP_REQUIRE(std::isfinite(dist[e]) && dist[e] >= 0.f, "tsne_affinities: dist[%lld] = %g", (long long)e, (double)dist[e]);
    DevBuf<float> dd, dp;
    GEMHIP_CHECK(dd.upload(dist, (size_t)n * k));
    GEMHIP_CHECK(dp.reserve((size_t)n * k));
    hipLaunchKernelGGL(tsne_affinity_kernel, dim3(grid_of(n, 4)), dim3(256), 0, 0, dd.get(), n, k, perplexity, dp.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(hipMemcpy(p_out, dp, (size_t)n * k * sizeof(float), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}
