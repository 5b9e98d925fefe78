// nc.hip -- node classification on the device: one-vs-rest L2 logistic regression on embedding rows by damped Newton,
// the top-k ranker and its per-class TP / FP / FN counts.  The host arithmetic (label check, Newton step, line search) is nc_host.hip.
//
// Kernels
//   nc_newton_pass_kernel  for a block of NC_CB classes and the gathered training rows x~_i = (x_i, 1): the loss sum, the gradient sums
//                          X~^T R and per class the upper-triangle 32 x 32 tiles of X~^T diag(s) X~ on v_mfma_f32_32x32x2_f32.
//   nc_loss_kernel         the loss sums alone at a block of trial points (the line search).
//   nc_reduce_kernel       the workgroups' partial sums in workgroup order, fp64.
//   nc_scores_kernel       logits of a row list against all K classes, fp64.
//   nc_topk_kernel         per row the k largest logits (ties: lower class id), the optional 0/1 prediction, integer-atomic counts.
//
// Numerics.  The logits, sigma, the residual r = p - Y, the weight s = p (1 - p) and the loss terms are fp64 (r and s in the forms that do
// not cancel where sigma saturates); the gradient sums are fp64 FMAs.  Only the Hessian runs in fp32: s is rounded once, the product
// s * x once, an MFMA chain covers NC_INNER = 32 rows, the chains of a super-slab of NC_CHAIN = 512 rows are added up in fp32 (16 adds) and
// the sum goes into the workgroup's fp64 partial tile.  The two levels are for the diagonal: its terms x^2 s all have one sign, and one
// fp32 chain of 1024 such terms was measured at up to 7.6e-7 of their sum (a random walk of roundings that grow with the partial sum,
// about 1.2e-7 * sqrt(L / 36) for a chain of L), where the mixed-sign chains the 1.5e-7 figure was quoted for stay far below.  There are
// no floating-point atomics: a workgroup owns a fixed set of row slabs and its own partials, nc_reduce_kernel adds the workgroups in order,
// and the grid is a function of n_train alone -- the same bits on every run.
//
// A workgroup (256 threads) takes super-slabs of NC_CHAIN rows, strided by the grid.  A super-slab goes through LDS in sub-slabs of NC_SUB
// rows, padded with zero rows and columns to the 32-wide tile; every (class, tile) pair of the block has its accumulator in some wave's
// registers, NC_NACC pairs per wave and round, the sub-slabs re-staged once per round.
//
// Limits (GEMHIP_E_UNSUPPORTED, refused on the host before any device call):
//   d  <= NC_MAX_D = 255    one thread per padded column of x~ and one LDS sub-slab of 64 x 256 floats
//   K  <= NC_MAX_K = 65536  the top-k kernel walks a row's K logits once per predicted label
//   n  <  2^31              row ids are int32; a row list (n_train, m) is below 2^31 too
#include "eval_common.hpp"
#include "nc_device.hpp"
#include "nc_host.hpp"
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>
#include <vector>

using namespace gemhip;

struct gemhip_nc {
    int64_t n = 0, ld = 0;
    int d = 0, d1 = 0, dp = 0, K = 0;
    bool have_labels = false, have_w = false;
    std::vector<int64_t> lab_ptr;
    std::vector<int32_t> lab_cls;
    std::vector<double> W;                                  // [K][d1], what prediction uses
    DevBuf<float> X;
    DevBuf<int64_t> d_lab_ptr;
    DevBuf<int32_t> d_lab_cls, d_idx, d_cls_ids, d_k;
    DevBuf<double> d_W, d_Wblk, partF, partG, partH, outF, outG, outH, d_scores;
    DevBuf<uint8_t> d_pred;
    DevBuf<unsigned long long> d_counts;
    Stopwatch watch;
    double ms[4] = {0, 0, 0, 0};                            // upload, fit, mean pass, predict
    int64_t passes = 0, loss_calls = 0, iterations = 0;
};

namespace {

constexpr int NC_CB = 4;             // classes per block
constexpr int NC_SUB = 64;           // rows per LDS sub-slab
constexpr int NC_CHAIN = 512;        // rows per super-slab: what a workgroup sums in fp32 before it adds into its fp64 partial
constexpr int NC_INNER = 32;         // rows per MFMA chain; the chains of a super-slab are then added up in fp32, NC_CHAIN / NC_INNER adds
constexpr int NC_NACC = 8;           // (class, tile) accumulators per wave and round
constexpr int NC_THREADS = 256;
constexpr int NC_MAXWG = 256;        // one workgroup per CU: the pass kernel's registers leave room for one wave per SIMD
constexpr int NC_MAX_D = 255;
constexpr int NC_MAX_K = 65536;
constexpr int64_t NC_SCORE_CHUNK = (int64_t)1 << 24;        // logits held on the device at a time

typedef float f32x16 __attribute__((ext_vector_type(16)));

size_t nc_lds_bytes(int dp)
{
    return sizeof(double) * ((size_t)NC_SUB * NC_CB + (size_t)NC_CB * dp + NC_THREADS) + sizeof(float) * ((size_t)NC_SUB * (dp + 1) + (size_t)NC_CHAIN * NC_CB);
}

// Is class `want` among the labels of `node`?  Rows are short and unsorted.
__device__ __forceinline__ bool nc_has_label(const int64_t *__restrict__ lab_ptr, const int32_t *__restrict__ lab_cls, int64_t node, int want)
{
    bool y = false;
    for (int64_t e = lab_ptr[node]; e < lab_ptr[node + 1]; ++e) y = y || lab_cls[e] == want;
    return y;
}

// Rows [first, first + NC_SUB) of the gathered, padded x~ into Xs [NC_SUB][ldx]: columns < d from X, column d = 1, the rest and every row
// past row_end zero.  A wave takes rows wave, wave + 4, ...; its lanes the columns: coalesced 256-byte reads.  The sixteen row ids first, then
// sixteen row segments in flight per 64 columns: with one wave per SIMD nothing else hides the gathered rows' latency.
__device__ __forceinline__ void nc_stage(float *Xs, int ldx, const float *__restrict__ X, int64_t ld, int d, int dp, const int32_t *__restrict__ idx, int64_t first,
                                         int64_t row_end)
{
    constexpr int RPW = NC_SUB / (NC_THREADS / 64);                      // rows per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t base[RPW];
    bool live[RPW];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        const int64_t gr = first + wave + q * (NC_THREADS / 64);
        live[q] = gr < row_end;
        base[q] = live[q] ? (int64_t)idx[gr] * ld : 0;
    }
    for (int j = lane; j < dp; j += 64) {
        float v[RPW];
#pragma unroll
        for (int q = 0; q < RPW; ++q) v[q] = !live[q] ? 0.f : j < d ? X[base[q] + j] : j == d ? 1.f : 0.f;
#pragma unroll
        for (int q = 0; q < RPW; ++q) Xs[(wave + q * (NC_THREADS / 64)) * ldx + j] = v[q];
    }
}

// The body of nc_newton_pass_kernel (WANT_GH) and nc_loss_kernel (!WANT_GH).
// W [NC_CB][dp] fp64: w, b at column d, zeros after.  cls_ids [NC_CB]: the block's class ids, ncls of them live.
// partF [grid][NC_CB], partG [grid][NC_CB][dp], partH [grid][NC_CB * ntri][32][32]: this workgroup's slices are written whole.
template <bool WANT_GH>
__device__ __forceinline__ void nc_pass_body(const float *__restrict__ X, int64_t ld, int d, int dp, const int32_t *__restrict__ idx, int64_t n_train,
                                             const int64_t *__restrict__ lab_ptr, const int32_t *__restrict__ lab_cls, const int32_t *__restrict__ cls_ids, int ncls,
                                             const double *__restrict__ W, double *__restrict__ partF, double *__restrict__ partG, double *__restrict__ partH)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char nc_lds[];
    double *r_sub = reinterpret_cast<double *>(nc_lds);                  // [NC_SUB][NC_CB]
    double *Wd = r_sub + NC_SUB * NC_CB;                                 // [NC_CB][dp]
    double *red = Wd + NC_CB * dp;                                       // [NC_THREADS]
    float *Xs = reinterpret_cast<float *>(red + NC_THREADS);             // [NC_SUB][ldx]
    const int ldx = dp + 1;                                              // odd stride: the logit loop's 16 rows per wave fall into 16 banks
    float *s_all = Xs + NC_SUB * ldx;                                    // [NC_CHAIN][NC_CB]

    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int T = dp >> 5, ntri = T * (T + 1) / 2, npairs = ncls * ntri;
    const int nrounds = (npairs + 4 * NC_NACC - 1) / (4 * NC_NACC);
    const int64_t nsuper = (n_train + NC_CHAIN - 1) / NC_CHAIN;

    for (int q = tid; q < NC_CB * dp; q += NC_THREADS) Wd[q] = W[q];
    const int my_r = tid >> 2, my_c = tid & 3;
    const int my_cls = my_c < ncls ? cls_ids[my_c] : -1;
    double facc = 0.0;
    double gacc[NC_CB] = {0.0, 0.0, 0.0, 0.0};

    for (int64_t ss = blockIdx.x; ss < nsuper; ss += gridDim.x) {
        const int64_t row0 = ss * NC_CHAIN;
        const int64_t row_end = row0 + NC_CHAIN < n_train ? row0 + NC_CHAIN : n_train;
        const int nsub = (int)((row_end - row0 + NC_SUB - 1) / NC_SUB);
        // ---- logits, residuals, weights, loss, gradient
        for (int sb = 0; sb < nsub; ++sb) {
            __syncthreads();                                             // the last readers of Xs, r_sub (and Wd's writers) are through
            nc_stage(Xs, ldx, X, ld, d, dp, idx, row0 + (int64_t)sb * NC_SUB, row_end);
            __syncthreads();
            {
                const int64_t gr = row0 + (int64_t)sb * NC_SUB + my_r;
                float sv = 0.f;
                double rv = 0.0;
                if (gr < row_end && my_cls >= 0) {
                    double z = 0.0;
                    for (int j = 0; j <= d; ++j) z += (double)Xs[my_r * ldx + j] * Wd[my_c * dp + j];
                    const bool y = nc_has_label(lab_ptr, lab_cls, idx[gr], my_cls);
                    const double e = exp(-fabs(z)), t = 1.0 / (1.0 + e);
                    const double p = z >= 0.0 ? t : e * t, q = z >= 0.0 ? e * t : t;          // sigma(z), 1 - sigma(z)
                    rv = y ? -q : p;
                    sv = (float)(e * t * t);
                    facc += log1p(e) + (y ? fmax(-z, 0.0) : fmax(z, 0.0));
                }
                if (WANT_GH) {
                    s_all[(sb * NC_SUB + my_r) * NC_CB + my_c] = sv;
                    r_sub[my_r * NC_CB + my_c] = rv;
                }
            }
            if (WANT_GH) {
                __syncthreads();
                if (tid < dp)
                    for (int r = 0; r < NC_SUB; ++r) {
                        const double x = (double)Xs[r * ldx + tid];
#pragma unroll
                        for (int c = 0; c < NC_CB; ++c) gacc[c] = fma(x, r_sub[r * NC_CB + c], gacc[c]);
                    }
            }
        }
        // ---- Hessian tiles
        if (WANT_GH)
            for (int rd = 0; rd < nrounds; ++rd) {
                int offa[NC_NACC], offb[NC_NACC], cls[NC_NACC], pair[NC_NACC];
#pragma unroll
                for (int a = 0; a < NC_NACC; ++a) {
                    const int p = (rd * 4 + wave) * NC_NACC + a;
                    pair[a] = p < npairs ? p : -1;
                    const int c = p < npairs ? p / ntri : 0;
                    int tri = p < npairs ? p - c * ntri : 0, ti = 0;
                    while (tri >= T - ti) { tri -= T - ti; ++ti; }                            // row-major upper triangle: row ti has T - ti tiles
                    cls[a] = c; offa[a] = ti * 32 + l31; offb[a] = (ti + tri) * 32 + l31;
                }
                f32x16 acc[NC_NACC];
#pragma unroll
                for (int a = 0; a < NC_NACC; ++a)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[a][q] = 0.f;
                for (int sb = 0; sb < nsub; ++sb) {
                    __syncthreads();
                    nc_stage(Xs, ldx, X, ld, d, dp, idx, row0 + (int64_t)sb * NC_SUB, row_end);
                    __syncthreads();
                    for (int k0 = 0; k0 < NC_SUB; k0 += NC_INNER) {               // two levels: a chain of NC_INNER rows, then one add per chain
                        f32x16 in[NC_NACC];
#pragma unroll
                        for (int a = 0; a < NC_NACC; ++a)
#pragma unroll
                            for (int q = 0; q < 16; ++q) in[a][q] = 0.f;
#pragma unroll 2
                        for (int k = k0; k < k0 + NC_INNER; k += 2) {
                            const float *xr = Xs + (k + h) * ldx;
                            const float *sr = s_all + (sb * NC_SUB + k + h) * NC_CB;
                            float av[NC_NACC], bv[NC_NACC];                      // (a slot without a pair repeats pair 0's tile and is dropped below: no branch here)
#pragma unroll
                            for (int a = 0; a < NC_NACC; ++a) { av[a] = xr[offa[a]] * sr[cls[a]]; bv[a] = xr[offb[a]]; }
#pragma unroll
                            for (int a = 0; a < NC_NACC; ++a) in[a] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[a], bv[a], in[a], 0, 0, 0);
                        }
#pragma unroll
                        for (int a = 0; a < NC_NACC; ++a) acc[a] += in[a];
                    }
                }
                const bool first = ss == (int64_t)blockIdx.x;
#pragma unroll
                for (int a = 0; a < NC_NACC; ++a)
                    if (pair[a] >= 0) {
                        double *dst = partH + ((size_t)blockIdx.x * (NC_CB * ntri) + pair[a]) * 1024;
                        double old[16];                                                      // all sixteen loads in flight, then the stores
#pragma unroll
                        for (int q = 0; q < 16; ++q) old[q] = first ? 0.0 : dst[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + l31];      // C/D map of the 32 x 32 MFMA
#pragma unroll
                        for (int q = 0; q < 16; ++q) dst[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + l31] = old[q] + (double)acc[a][q];
                    }
            }
    }
    // ---- this workgroup's sums
    __syncthreads();
    red[tid] = facc;
    __syncthreads();
    if (tid < NC_CB) {
        double s = 0.0;
        for (int r = 0; r < NC_SUB; ++r) s += red[r * NC_CB + tid];
        partF[(size_t)blockIdx.x * NC_CB + tid] = s;
    }
    if (WANT_GH && tid < dp)
#pragma unroll
        for (int c = 0; c < NC_CB; ++c) partG[((size_t)blockIdx.x * NC_CB + c) * dp + tid] = gacc[c];
}

__global__ __launch_bounds__(NC_THREADS) void nc_newton_pass_kernel(const float *__restrict__ X, int64_t ld, int d, int dp, const int32_t *__restrict__ idx,
                                                                    int64_t n_train, const int64_t *__restrict__ lab_ptr, const int32_t *__restrict__ lab_cls,
                                                                    const int32_t *__restrict__ cls_ids, int ncls, const double *__restrict__ W,
                                                                    double *__restrict__ partF, double *__restrict__ partG, double *__restrict__ partH)
{
    nc_pass_body<true>(X, ld, d, dp, idx, n_train, lab_ptr, lab_cls, cls_ids, ncls, W, partF, partG, partH);
}

// W holds each class's own trial point theta_c + alpha_c delta_c (nc_trial_point).
__global__ __launch_bounds__(NC_THREADS) void nc_loss_kernel(const float *__restrict__ X, int64_t ld, int d, int dp, const int32_t *__restrict__ idx, int64_t n_train,
                                                             const int64_t *__restrict__ lab_ptr, const int32_t *__restrict__ lab_cls,
                                                             const int32_t *__restrict__ cls_ids, int ncls, const double *__restrict__ W, double *__restrict__ partF)
{
    nc_pass_body<false>(X, ld, d, dp, idx, n_train, lab_ptr, lab_cls, cls_ids, ncls, W, partF, nullptr, nullptr);
}

// out[i] = part[0][i] + part[1][i] + ... in that order, i < count; part g begins at g * stride.
__global__ void nc_reduce_kernel(const double *__restrict__ part, int nparts, int64_t stride, int64_t count, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    double s = 0.0;
    for (int g = 0; g < nparts; ++g) s += part[(size_t)g * stride + i];
    out[i] = s;
}

// out[r][c] = x_{idx[first + r]} . w_c + b_c, W [K][d1].
__global__ void nc_scores_kernel(const float *__restrict__ X, int64_t ld, int d, const int32_t *__restrict__ idx, int64_t first, int64_t rows, int K,
                                 const double *__restrict__ W, double *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= rows * K) return;
    const int64_t r = q / K;
    const int c = (int)(q - r * K);
    const float *px = X + (int64_t)idx[first + r] * ld;
    const double *w = W + (size_t)c * (d + 1);
    double z = 0.0;
    for (int j = 0; j < d; ++j) z = fma((double)px[j], w[j], z);
    out[q] = z + w[d];
}

// One thread per row: the k largest of its K logits, the earlier class on equal logits.  pred [rows][K] is scratch and result (0 / 1).
// counts [3][K]: TP, FP, FN per class; counts[3 * K]: rows whose predicted set is the true set.
__global__ void nc_topk_kernel(const double *__restrict__ scores, int64_t rows, int K, const int32_t *__restrict__ idx, int64_t first, const int32_t *__restrict__ k_arr,
                               const int64_t *__restrict__ lab_ptr, const int32_t *__restrict__ lab_cls, uint8_t *__restrict__ pred,
                               unsigned long long *__restrict__ counts)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int64_t node = idx[first + r];
    const int64_t e0 = lab_ptr[node], e1 = lab_ptr[node + 1];
    int k = k_arr ? k_arr[first + r] : (int)(e1 - e0);
    k = k < 0 ? 0 : k > K ? K : k;                                       // (the host has refused k outside [0, K])
    const double *sc = scores + (size_t)r * K;
    uint8_t *pr = pred + (size_t)r * K;
    for (int c = 0; c < K; ++c) pr[c] = 0;
    for (int t = 0; t < k; ++t) {
        int best = -1;
        double bv = 0.0;
        for (int c = 0; c < K; ++c)
            if (!pr[c] && (best < 0 || sc[c] > bv)) { best = c; bv = sc[c]; }
        pr[best] = 1;
    }
    int wrong = 0;
    for (int64_t e = e0; e < e1; ++e) {
        const int c = lab_cls[e];
        if (pr[c]) { atomicAdd(&counts[c], 1ull); pr[c] = 2; }
        else { atomicAdd(&counts[2 * (size_t)K + c], 1ull); ++wrong; }
    }
    for (int c = 0; c < K; ++c) {
        if (pr[c] == 1) { atomicAdd(&counts[(size_t)K + c], 1ull); ++wrong; }
        else if (pr[c] == 2) pr[c] = 1;
    }
    if (!wrong) atomicAdd(&counts[3 * (size_t)K], 1ull);
}

// ================================================================== host side
int check_rows(const char *who, const gemhip_nc *h, int64_t m, const int32_t *idx)
{
    GEMHIP_REQUIRE(m >= 1, "%s: %lld rows (need >= 1)", who, (long long)m);
    GEMHIP_REQUIRE(idx != nullptr, "%s: NULL row list", who);
    if (m > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "%s: %lld rows: must be below 2^31", who, (long long)m);
    const int64_t bad = first_bad_index(idx, m, h->n);
    GEMHIP_REQUIRE(bad < 0, "%s: row %lld = %d outside [0,%lld)", who, (long long)bad, idx[bad], (long long)h->n);
    return GEMHIP_OK;
}

int set_lds_limit(int dp)
{
    const int bytes = (int)nc_lds_bytes(dp);
    GEMHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(nc_newton_pass_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    GEMHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(nc_loss_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return GEMHIP_OK;
}

// The sums of one pass (want_gh) or loss evaluation over h->d_idx[0 .. n_train) for the classes `ids`, at W_rows[q] (d1 doubles each).
// loss [nq]; gsum [nq][dp] and tiles [nq][ntri][1024] with want_gh.  Blocks of NC_CB classes, enqueued back to back, one copy back.
int run_pass(gemhip_nc *h, int64_t n_train, const std::vector<int32_t> &ids, const std::vector<const double *> &W_rows, bool want_gh, std::vector<double> &loss,
             std::vector<double> &gsum, std::vector<double> &tiles)
{
    const int nq = (int)ids.size(), dp = h->dp, d1 = h->d1, T = dp / 32, ntri = T * (T + 1) / 2;
    if (!nq) return GEMHIP_OK;
    const int nblocks = (nq + NC_CB - 1) / NC_CB;
    const int64_t nsuper = (n_train + NC_CHAIN - 1) / NC_CHAIN;
    const int grid = (int)(nsuper < NC_MAXWG ? nsuper : NC_MAXWG);
    const size_t lds = nc_lds_bytes(dp);
    std::vector<double> wblk((size_t)nblocks * NC_CB * dp, 0.0);
    std::vector<int32_t> cid((size_t)nblocks * NC_CB, -1);
    for (int q = 0; q < nq; ++q) {
        cid[q] = ids[q];
        for (int j = 0; j < d1; ++j) wblk[(size_t)q * dp + j] = W_rows[q][j];
    }
    GEMHIP_CHECK(h->d_Wblk.upload(wblk.data(), wblk.size()));
    GEMHIP_CHECK(h->d_cls_ids.upload(cid.data(), cid.size()));
    GEMHIP_CHECK(h->partF.reserve((size_t)grid * NC_CB));
    GEMHIP_CHECK(h->outF.reserve((size_t)nblocks * NC_CB));
    if (want_gh) {
        GEMHIP_CHECK(h->partG.reserve((size_t)grid * NC_CB * dp));
        GEMHIP_CHECK(h->partH.reserve((size_t)grid * NC_CB * ntri * 1024));
        GEMHIP_CHECK(h->outG.reserve((size_t)nblocks * NC_CB * dp));
        GEMHIP_CHECK(h->outH.reserve((size_t)nblocks * NC_CB * ntri * 1024));
    }
    for (int b = 0; b < nblocks; ++b) {
        const int ncls = nq - b * NC_CB < NC_CB ? nq - b * NC_CB : NC_CB;
        const double *Wb = h->d_Wblk.get() + (size_t)b * NC_CB * dp;
        const int32_t *cb = h->d_cls_ids.get() + (size_t)b * NC_CB;
        if (want_gh) {
            hipLaunchKernelGGL(nc_newton_pass_kernel, dim3(grid), dim3(NC_THREADS), lds, 0, h->X.get(), h->ld, h->d, dp, h->d_idx.get(), n_train, h->d_lab_ptr.get(),
                               h->d_lab_cls.get(), cb, ncls, Wb, h->partF.get(), h->partG.get(), h->partH.get());
            const int64_t cg = (int64_t)NC_CB * dp, ch = (int64_t)NC_CB * ntri * 1024;
            hipLaunchKernelGGL(nc_reduce_kernel, dim3(grid_of(cg, 256)), dim3(256), 0, 0, h->partG.get(), grid, cg, cg, h->outG.get() + (size_t)b * cg);
            // (a workgroup's stride in partH is NC_CB * ntri tiles whatever ncls is; only the live pairs were written, only they are summed)
            hipLaunchKernelGGL(nc_reduce_kernel, dim3(grid_of((int64_t)ncls * ntri * 1024, 256)), dim3(256), 0, 0, h->partH.get(), grid, ch,
                               (int64_t)ncls * ntri * 1024, h->outH.get() + (size_t)b * ch);
        } else {
            hipLaunchKernelGGL(nc_loss_kernel, dim3(grid), dim3(NC_THREADS), lds, 0, h->X.get(), h->ld, h->d, dp, h->d_idx.get(), n_train, h->d_lab_ptr.get(),
                               h->d_lab_cls.get(), cb, ncls, Wb, h->partF.get());
        }
        hipLaunchKernelGGL(nc_reduce_kernel, dim3(1), dim3(256), 0, 0, h->partF.get(), grid, (int64_t)NC_CB, (int64_t)NC_CB, h->outF.get() + (size_t)b * NC_CB);
    }
    GEMHIP_CHECK(hipGetLastError());
    loss.resize((size_t)nblocks * NC_CB);
    GEMHIP_CHECK(hipMemcpy(loss.data(), h->outF, loss.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (want_gh) {
        gsum.resize((size_t)nblocks * NC_CB * dp);
        tiles.resize((size_t)nq * ntri * 1024);
        GEMHIP_CHECK(hipMemcpy(gsum.data(), h->outG, gsum.size() * sizeof(double), hipMemcpyDeviceToHost));
        GEMHIP_CHECK(hipMemcpy(tiles.data(), h->outH, tiles.size() * sizeof(double), hipMemcpyDeviceToHost));
        ++h->passes;
    } else
        ++h->loss_calls;
    return GEMHIP_OK;
}

// Upload a row list to h->d_idx.
int upload_rows(gemhip_nc *h, int64_t m, const int32_t *idx)
{
    GEMHIP_CHECK(h->d_idx.upload(idx, (size_t)m));
    return GEMHIP_OK;
}

int require_labels(const char *who, const gemhip_nc *h)
{
    GEMHIP_REQUIRE(h != nullptr, "%s: NULL handle", who);
    GEMHIP_REQUIRE(h->have_labels, "%s: no labels set (gemhip_nc_set_labels)", who);
    return GEMHIP_OK;
}

int check_C(const char *who, double C)
{
    GEMHIP_REQUIRE(std::isfinite(C) && C > 0.0, "%s: C = %g (need a finite C > 0)", who, C);
    return GEMHIP_OK;
}

// Logits of rows [first, first + rows) of h->d_idx into h->d_scores.
void enqueue_scores(gemhip_nc *h, int64_t first, int64_t rows)
{
    hipLaunchKernelGGL(nc_scores_kernel, dim3(grid_of(rows * h->K, 256)), dim3(256), 0, 0, h->X.get(), h->ld, h->d, h->d_idx.get(), first, rows, h->K, h->d_W.get(),
                       h->d_scores.get());
}

int64_t score_chunk(const gemhip_nc *h, int64_t m)
{
    const int64_t c = NC_SCORE_CHUNK / h->K;
    return c < 1 ? 1 : c < m ? c : m;
}

}  // namespace

extern "C" int gemhip_nc_create(int64_t n, int32_t d, int32_t ld, const float *X_host, gemhip_nc_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "nc_create: NULL output");
    *out = nullptr;
    int rc = check_embedding("nc_create", n, d, ld, X_host, 1, NC_MAX_D, "one LDS slab of the padded rows");
    if (rc) return rc;
    const int64_t bad = first_bad_entry(X_host, n, d, ld, INFINITY);
    GEMHIP_REQUIRE(bad < 0, "nc_create: X[%lld][%d] is not finite", (long long)(bad / d), (int)(bad % d));
    std::unique_ptr<gemhip_nc> h(new gemhip_nc);
    h->n = n; h->ld = ld; h->d = d; h->d1 = d + 1; h->dp = (d + 1 + 31) & ~31;
    const double t0 = wall_ms();
    GEMHIP_CHECK(h->X.upload(X_host, (size_t)n * ld));
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->ms[0] = wall_ms() - t0;
    if ((rc = set_lds_limit(h->dp))) return rc;
    *out = h.release();
    return GEMHIP_OK;
}

// nc_device.hpp: the same handle from a matrix on the device.  Additive: gemhip_nc_create above keeps its own path.
int gemhip::nc_create_from_device(int64_t n, int32_t d, int64_t ld, const float *X_dev, gemhip_nc_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "nc_create_from_device: NULL output");
    *out = nullptr;
    int rc = check_embedding("nc_create_from_device", n, d, ld, X_dev, 1, NC_MAX_D, "one LDS slab of the padded rows");
    if (rc) return rc;
    std::unique_ptr<gemhip_nc> h(new gemhip_nc);
    h->n = n; h->ld = ld; h->d = d; h->d1 = d + 1; h->dp = (d + 1 + 31) & ~31;
    const double t0 = wall_ms();
    GEMHIP_CHECK(h->X.reserve((size_t)n * ld));
    GEMHIP_CHECK(hipMemcpy(h->X, X_dev, (size_t)n * ld * sizeof(float), hipMemcpyDeviceToDevice));
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->ms[0] = wall_ms() - t0;
    if ((rc = set_lds_limit(h->dp))) return rc;
    *out = h.release();
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_destroy(gemhip_nc_t h)
{
    delete h;
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_set_labels(gemhip_nc_t h, int32_t K, const int64_t *row_ptr, const int32_t *cls)
{
    GEMHIP_REQUIRE(h != nullptr, "nc_set_labels: NULL handle");
    GEMHIP_REQUIRE(K >= 1, "nc_set_labels: K = %d (need K >= 1)", K);
    if (K > NC_MAX_K) return fail(GEMHIP_E_UNSUPPORTED, "nc_set_labels: K = %d: at most %d classes", K, NC_MAX_K);
    GEMHIP_REQUIRE(row_ptr != nullptr, "nc_set_labels: NULL row_ptr");
    const NcLabelError err = check_label_csr(h->n, K, row_ptr, cls);
    switch (err.kind) {
    case NcLabelError::NONE: break;
    case NcLabelError::ROW_PTR_FIRST: return fail(GEMHIP_E_INVALID, "nc_set_labels: row_ptr[0] = %lld (need 0)", (long long)row_ptr[0]);
    case NcLabelError::ROW_PTR_DECREASES: return fail(GEMHIP_E_INVALID, "nc_set_labels: row_ptr decreases at row %lld", (long long)err.row);
    case NcLabelError::CLS_NULL: return fail(GEMHIP_E_INVALID, "nc_set_labels: NULL class list");
    case NcLabelError::CLASS_OUT_OF_RANGE:
        return fail(GEMHIP_E_INVALID, "nc_set_labels: entry %lld (row %lld) = class %d outside [0,%d)", (long long)err.index, (long long)err.row, err.cls, K);
    case NcLabelError::CLASS_REPEATED:
        return fail(GEMHIP_E_INVALID, "nc_set_labels: entry %lld (row %lld) lists class %d twice", (long long)err.index, (long long)err.row, err.cls);
    }
    if (row_ptr[h->n] > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "nc_set_labels: %lld label entries: must be below 2^31", (long long)row_ptr[h->n]);
    h->have_labels = false; h->have_w = false;
    h->K = K;
    h->lab_ptr.assign(row_ptr, row_ptr + h->n + 1);
    h->lab_cls.assign(cls, cls + row_ptr[h->n]);
    GEMHIP_CHECK(h->d_lab_ptr.upload(h->lab_ptr.data(), h->lab_ptr.size()));
    GEMHIP_CHECK(h->d_lab_cls.upload(h->lab_cls.data(), h->lab_cls.size()));
    h->have_labels = true;
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_set_weights(gemhip_nc_t h, const double *W)
{
    int rc = require_labels("nc_set_weights", h);
    if (rc) return rc;
    GEMHIP_REQUIRE(W != nullptr, "nc_set_weights: NULL W");
    for (int c = 0; c < h->K; ++c) {
        for (int j = 0; j < h->d; ++j) GEMHIP_REQUIRE(std::isfinite(W[(size_t)c * h->d1 + j]), "nc_set_weights: W[%d][%d] is not finite", c, j);
        GEMHIP_REQUIRE(!std::isnan(W[(size_t)c * h->d1 + h->d]), "nc_set_weights: the intercept of class %d is NaN", c);
    }
    h->W.assign(W, W + (size_t)h->K * h->d1);
    GEMHIP_CHECK(h->d_W.upload(h->W.data(), h->W.size()));
    h->have_w = true;
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_pass(gemhip_nc_t h, int64_t n_train, const int32_t *train_idx, double C, const double *W, double *F_out, double *g_out, double *H_out)
{
    int rc = require_labels("nc_pass", h);
    if (rc) return rc;
    if ((rc = check_C("nc_pass", C))) return rc;
    if ((rc = check_rows("nc_pass", h, n_train, train_idx))) return rc;
    GEMHIP_REQUIRE(W && F_out && g_out && H_out, "nc_pass: NULL argument");
    const int d1 = h->d1, dp = h->dp, T = dp / 32, ntri = T * (T + 1) / 2;
    for (size_t q = 0; q < (size_t)h->K * d1; ++q) GEMHIP_REQUIRE(std::isfinite(W[q]), "nc_pass: W[%lld][%d] is not finite", (long long)(q / d1), (int)(q % d1));
    if ((rc = upload_rows(h, n_train, train_idx))) return rc;
    std::vector<int32_t> ids((size_t)h->K);
    std::vector<const double *> rows((size_t)h->K);
    for (int c = 0; c < h->K; ++c) { ids[c] = c; rows[c] = W + (size_t)c * d1; }
    std::vector<double> loss, gsum, tiles;
    if ((rc = run_pass(h, n_train, ids, rows, true, loss, gsum, tiles))) return rc;
    for (int c = 0; c < h->K; ++c)
        nc_assemble(d1, dp, C, rows[c], loss[c], gsum.data() + (size_t)c * dp, tiles.data() + (size_t)c * ntri * 1024, F_out + c, g_out + (size_t)c * d1,
                    H_out + (size_t)c * d1 * d1);
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_newton_step_host(int32_t d1, const double *H, const double *g, double *delta_out, double *dec_out, double *shift_out)
{
    GEMHIP_REQUIRE(d1 >= 1 && H && g && delta_out && dec_out, "nc_newton_step_host: bad arguments");
    if (!nc_newton_step(d1, H, g, delta_out, dec_out, shift_out))
        return fail(GEMHIP_E_NOTCONVERGED, "nc_newton_step_host: no Levenberg shift made H positive definite (or H, g are not finite)");
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_fit(gemhip_nc_t h, int64_t n_train, const int32_t *train_idx, double C, double dec_tol, int32_t max_iter, double *W_inout, double *info_out)
{
    int rc = require_labels("nc_fit", h);
    if (rc) return rc;
    if ((rc = check_C("nc_fit", C))) return rc;
    GEMHIP_REQUIRE(std::isfinite(dec_tol) && dec_tol > 0.0, "nc_fit: dec_tol = %g (need a finite dec_tol > 0)", dec_tol);
    GEMHIP_REQUIRE(max_iter >= 1, "nc_fit: max_iter = %d (need >= 1)", max_iter);
    if ((rc = check_rows("nc_fit", h, n_train, train_idx))) return rc;
    GEMHIP_REQUIRE(W_inout != nullptr, "nc_fit: NULL W");
    const int K = h->K, d1 = h->d1, dp = h->dp, T = dp / 32, ntri = T * (T + 1) / 2;
    const std::vector<int64_t> pos = nc_class_positives(K, h->lab_ptr.data(), h->lab_cls.data(), n_train, train_idx);
    std::vector<NcClass> cls((size_t)K);
    for (int c = 0; c < K; ++c) {
        cls[c].id = c;
        cls[c].degenerate = nc_degenerate(pos[c], n_train);
        cls[c].theta.assign(W_inout + (size_t)c * d1, W_inout + (size_t)(c + 1) * d1);
        if (cls[c].degenerate) {
            cls[c].theta.assign((size_t)d1, 0.0);
            cls[c].theta[d1 - 1] = cls[c].degenerate < 0 ? -std::numeric_limits<double>::infinity() : std::numeric_limits<double>::infinity();
        } else
            for (int j = 0; j < d1; ++j) GEMHIP_REQUIRE(std::isfinite(cls[c].theta[j]), "nc_fit: the start W[%d][%d] is not finite", c, j);
    }
    if ((rc = upload_rows(h, n_train, train_idx))) return rc;
    h->passes = 0; h->loss_calls = 0; h->iterations = 0;
    const double t0 = wall_ms();
    double pass_ms = 0.0;
    std::vector<double> loss, gsum, tiles, none_g, none_h, g((size_t)d1), H((size_t)d1 * d1), trial;
    for (int it = 0; it < max_iter; ++it) {
        std::vector<int32_t> active;
        for (int c = 0; c < K; ++c)
            if (!cls[c].degenerate && !cls[c].converged && !cls[c].stopped) active.push_back(c);
        if (active.empty()) break;
        ++h->iterations;
        std::vector<const double *> rows;
        for (int32_t c : active) rows.push_back(cls[c].theta.data());
        const double tp = wall_ms();
        if ((rc = run_pass(h, n_train, active, rows, true, loss, gsum, tiles))) return rc;
        pass_ms += wall_ms() - tp;
        std::vector<int32_t> search;                                       // classes whose trial point still needs its loss
        for (size_t q = 0; q < active.size(); ++q) {
            NcClass &c = cls[active[q]];
            double F = 0.0;
            nc_assemble(d1, dp, C, c.theta.data(), loss[q], gsum.data() + q * dp, tiles.data() + q * ntri * 1024, &F, g.data(), H.data());
            if (nc_begin_step(c, d1, F, g.data(), H.data())) search.push_back(c.id);
            else if (!c.stopped) nc_accept_step(c, d1, dec_tol);
        }
        while (!search.empty()) {
            trial.resize(search.size() * (size_t)d1);
            rows.clear();
            for (size_t q = 0; q < search.size(); ++q) {
                nc_trial_point(cls[search[q]], d1, trial.data() + q * d1);
                rows.push_back(trial.data() + q * d1);
            }
            if ((rc = run_pass(h, n_train, search, rows, false, loss, none_g, none_h))) return rc;
            std::vector<int32_t> again;
            for (size_t q = 0; q < search.size(); ++q) {
                NcClass &c = cls[search[q]];
                double w2 = 0.0;
                for (int j = 0; j < d1 - 1; ++j) w2 += trial[q * d1 + j] * trial[q * d1 + j];
                const NcTrial verdict = nc_judge_trial(c, C * loss[q] + 0.5 * w2);
                if (verdict == NC_ACCEPT) nc_accept_step(c, d1, dec_tol);
                else if (verdict == NC_RETRY) again.push_back(c.id);
            }
            search.swap(again);
        }
    }
    h->ms[1] = wall_ms() - t0;
    h->ms[2] = h->passes ? pass_ms / (double)h->passes : 0.0;
    for (int c = 0; c < K; ++c) {
        for (int j = 0; j < d1; ++j) W_inout[(size_t)c * d1 + j] = cls[c].theta[j];
        if (info_out) {
            double *o = info_out + (size_t)c * 6;
            o[0] = cls[c].iterations; o[1] = cls[c].backtracks; o[2] = cls[c].gmax; o[3] = cls[c].dec;
            o[4] = cls[c].degenerate || cls[c].converged ? 1.0 : 0.0; o[5] = cls[c].degenerate;
        }
    }
    h->W.assign(W_inout, W_inout + (size_t)K * d1);
    GEMHIP_CHECK(h->d_W.upload(h->W.data(), h->W.size()));
    h->have_w = true;
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_scores(gemhip_nc_t h, int64_t m, const int32_t *idx, double *out)
{
    int rc = require_labels("nc_scores", h);
    if (rc) return rc;
    GEMHIP_REQUIRE(h->have_w, "nc_scores: no weights (gemhip_nc_fit or gemhip_nc_set_weights)");
    if ((rc = check_rows("nc_scores", h, m, idx))) return rc;
    GEMHIP_REQUIRE(out != nullptr, "nc_scores: NULL output");
    if ((rc = upload_rows(h, m, idx))) return rc;
    const int64_t chunk = score_chunk(h, m);
    GEMHIP_CHECK(h->d_scores.reserve((size_t)chunk * h->K));
    for (int64_t first = 0; first < m; first += chunk) {
        const int64_t rows = first + chunk < m ? chunk : m - first;
        enqueue_scores(h, first, rows);
        GEMHIP_CHECK(hipGetLastError());
        GEMHIP_CHECK(hipMemcpy(out + (size_t)first * h->K, h->d_scores, (size_t)rows * h->K * sizeof(double), hipMemcpyDeviceToHost));
    }
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_predict_topk(gemhip_nc_t h, int64_t m, const int32_t *idx, const int32_t *k_or_null, uint8_t *pred_or_null, int64_t *counts_out,
                                      int64_t *exact_out)
{
    int rc = require_labels("nc_predict_topk", h);
    if (rc) return rc;
    GEMHIP_REQUIRE(h->have_w, "nc_predict_topk: no weights (gemhip_nc_fit or gemhip_nc_set_weights)");
    if ((rc = check_rows("nc_predict_topk", h, m, idx))) return rc;
    GEMHIP_REQUIRE(counts_out && exact_out, "nc_predict_topk: NULL output");
    const int K = h->K;
    if (k_or_null)
        for (int64_t t = 0; t < m; ++t) GEMHIP_REQUIRE(k_or_null[t] >= 0 && k_or_null[t] <= K, "nc_predict_topk: k[%lld] = %d outside [0,%d]", (long long)t, k_or_null[t], K);
    if ((rc = upload_rows(h, m, idx))) return rc;
    if (k_or_null) GEMHIP_CHECK(h->d_k.upload(k_or_null, (size_t)m));
    const int64_t chunk = score_chunk(h, m);
    GEMHIP_CHECK(h->d_scores.reserve((size_t)chunk * K));
    GEMHIP_CHECK(h->d_pred.reserve((size_t)chunk * K));
    GEMHIP_CHECK(h->d_counts.reserve((size_t)3 * K + 1));
    GEMHIP_CHECK(hipMemsetAsync(h->d_counts, 0, ((size_t)3 * K + 1) * sizeof(unsigned long long), 0));
    GEMHIP_CHECK(start(h->watch));
    for (int64_t first = 0; first < m; first += chunk) {
        const int64_t rows = first + chunk < m ? chunk : m - first;
        enqueue_scores(h, first, rows);
        hipLaunchKernelGGL(nc_topk_kernel, dim3(grid_of(rows, 64)), dim3(64), 0, 0, h->d_scores.get(), rows, K, h->d_idx.get(), first,
                           k_or_null ? h->d_k.get() : (const int32_t *)nullptr, h->d_lab_ptr.get(), h->d_lab_cls.get(), h->d_pred.get(), h->d_counts.get());
        GEMHIP_CHECK(hipGetLastError());
        if (pred_or_null) GEMHIP_CHECK(hipMemcpy(pred_or_null + (size_t)first * K, h->d_pred, (size_t)rows * K, hipMemcpyDeviceToHost));
    }
    GEMHIP_CHECK(stop(h->watch, &h->ms[3]));
    std::vector<unsigned long long> cnt((size_t)3 * K + 1);
    GEMHIP_CHECK(hipMemcpy(cnt.data(), h->d_counts, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < (size_t)3 * K; ++q) counts_out[q] = (int64_t)cnt[q];
    *exact_out = (int64_t)cnt[(size_t)3 * K];
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_last_ms(gemhip_nc_t h, double *out)
{
    GEMHIP_REQUIRE(h && out, "nc_last_ms: NULL");
    for (int q = 0; q < 4; ++q) out[q] = h->ms[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_nc_info(gemhip_nc_t h, int64_t *out)
{
    GEMHIP_REQUIRE(h && out, "nc_info: NULL");
    out[0] = h->n; out[1] = h->d; out[2] = h->K; out[3] = h->passes; out[4] = h->loss_calls; out[5] = h->iterations; out[6] = NC_CB; out[7] = NC_SUB;
    return GEMHIP_OK;
}
