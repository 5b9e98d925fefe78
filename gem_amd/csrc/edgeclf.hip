// edgeclf.hip -- link prediction as classification: the feature of a node pair from a binary operator on the two embedding
// rows (node2vec, section 4.4), the fused pair score, and the logistic fit on pair features through the node-classification solver.
//
// Kernels
//   ec_features_kernel  F[p] = op(X[st[p]], X[ed[p]]), m x d float32.
//   ec_scores_kernel    score[p] = sum_j (double)op(a, b)_j * w_j + w_d without forming F; w == NULL: sum_j (double)a_j * (double)b_j.
// A wavefront takes EC_PPW = 8 pairs at a time and its lanes take the columns: the sixteen row ids first, then sixteen row segments in flight
// per 64 columns, as nc_stage does -- nothing else hides the latency of the gathered rows.
//
// Numerics.  The operators are single fp32 operations or two that cannot contract (no FMA): (a + b) * 0.5f, a * b, fabsf(a - b) and
// t = a - b rounded, then t * t -- bit-equal to the same expressions in numpy float32.  The score widens the fp32 feature and adds fp64
// products per lane over its columns in ascending order, then the 64 lanes by a butterfly: a fixed order, no atomics, the same bits on every run.
//
// gemhip_edgeclf_fit needs 2 * m * d * 4 bytes of device memory at its peak: the m x d feature matrix and the copy of it the solver's handle
// owns (nc_create_from_device); the feature matrix is freed right after the copy, so the fit itself runs on m * d * 4 bytes.
//
// Limits, refused on the host before any device call: d <= 255 and n, m < 2^31 (GEMHIP_E_UNSUPPORTED); |X| <= 1e18 (GEMHIP_E_INVALID: every
// operator's result is then finite in fp32, which the solver requires of its matrix).
#include "eval_common.hpp"
#include "nc_device.hpp"
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace gemhip;

struct gemhip_edgeclf {
    int64_t n = 0, ld = 0;
    int d = 0;
    DevBuf<float> X, F;
    DevBuf<int32_t> st, ed;
    DevBuf<double> w, out;
    Stopwatch watch;
    double ms[6] = {0, 0, 0, 0, 0, 0};                      // upload, features, scores, fit, the fit's mean pass, the fit's feature kernel
    int64_t passes = 0, loss_calls = 0, iterations = 0, last_m = 0;
};

namespace {

constexpr int EC_THREADS = 256;
constexpr int EC_PPW = 8;                                    // pairs a wave has in flight
constexpr int EC_PAIRS_PER_WG = EC_PPW * (EC_THREADS / 64);
constexpr int EC_MAX_D = 255;
constexpr int EC_MAX_GRID = 8192;
constexpr float EC_MAX_ABS = 1e18f;
enum { EC_AVERAGE = 0, EC_HADAMARD = 1, EC_L1 = 2, EC_L2 = 3, EC_OPS = 4 };

__device__ __forceinline__ float ec_apply(int op, float a, float b)
{
#pragma clang fp contract(off)
    if (op == EC_AVERAGE) return (a + b) * 0.5f;
    if (op == EC_HADAMARD) return a * b;
    const float t = a - b;
    return op == EC_L1 ? fabsf(t) : t * t;
}

__global__ __launch_bounds__(EC_THREADS) void ec_features_kernel(const float *__restrict__ X, int64_t ld, int d, int op, const int32_t *__restrict__ st,
                                                                 const int32_t *__restrict__ ed, int64_t m, float *__restrict__ F)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (EC_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (EC_THREADS / 64);
    for (int64_t p0 = wave * EC_PPW; p0 < m; p0 += nwaves * EC_PPW) {
        int64_t ba[EC_PPW], bb[EC_PPW];
        bool live[EC_PPW];
#pragma unroll
        for (int q = 0; q < EC_PPW; ++q) {
            live[q] = p0 + q < m;
            ba[q] = live[q] ? (int64_t)st[p0 + q] * ld : 0;
            bb[q] = live[q] ? (int64_t)ed[p0 + q] * ld : 0;
        }
        for (int j = lane; j < d; j += 64) {
            float a[EC_PPW], b[EC_PPW];
#pragma unroll
            for (int q = 0; q < EC_PPW; ++q) {
                a[q] = live[q] ? X[ba[q] + j] : 0.f;
                b[q] = live[q] ? X[bb[q] + j] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < EC_PPW; ++q)
                if (live[q]) F[(p0 + q) * (int64_t)d + j] = ec_apply(op, a[q], b[q]);
        }
    }
}

// w [d + 1] or NULL.
__global__ __launch_bounds__(EC_THREADS) void ec_scores_kernel(const float *__restrict__ X, int64_t ld, int d, int op, const int32_t *__restrict__ st,
                                                               const int32_t *__restrict__ ed, int64_t m, const double *__restrict__ w, double *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (EC_THREADS / 64) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (EC_THREADS / 64);
    for (int64_t p0 = wave * EC_PPW; p0 < m; p0 += nwaves * EC_PPW) {
        int64_t ba[EC_PPW], bb[EC_PPW];
        bool live[EC_PPW];
        double acc[EC_PPW];
#pragma unroll
        for (int q = 0; q < EC_PPW; ++q) {
            live[q] = p0 + q < m;
            ba[q] = live[q] ? (int64_t)st[p0 + q] * ld : 0;
            bb[q] = live[q] ? (int64_t)ed[p0 + q] * ld : 0;
            acc[q] = 0.0;
        }
        for (int j = lane; j < d; j += 64) {
            float a[EC_PPW], b[EC_PPW];
#pragma unroll
            for (int q = 0; q < EC_PPW; ++q) {
                a[q] = live[q] ? X[ba[q] + j] : 0.f;
                b[q] = live[q] ? X[bb[q] + j] : 0.f;
            }
            const double wj = w ? w[j] : 0.0;
#pragma unroll
            for (int q = 0; q < EC_PPW; ++q) acc[q] += w ? (double)ec_apply(op, a[q], b[q]) * wj : (double)a[q] * (double)b[q];
        }
#pragma unroll
        for (int q = 0; q < EC_PPW; ++q) {
            const double s = wave_sum_f64(acc[q]);
            if (lane == 0 && live[q]) out[p0 + q] = w ? s + w[d] : s;
        }
    }
}

unsigned ec_grid(int64_t m) { return std::min<unsigned>(grid_of(m, EC_PAIRS_PER_WG), EC_MAX_GRID); }

int check_pairs(const char *who, const gemhip_edgeclf *h, int op, bool op_matters, int64_t m, const int32_t *st, const int32_t *ed)
{
    GEMHIP_REQUIRE(h != nullptr, "%s: NULL handle", who);
    if (op_matters) GEMHIP_REQUIRE(op >= 0 && op < EC_OPS, "%s: operator %d outside [0,%d) (0 average, 1 Hadamard, 2 L1, 3 L2)", who, op, (int)EC_OPS);
    GEMHIP_REQUIRE(m >= 1, "%s: m = %lld pairs (need m >= 1)", who, (long long)m);
    if (m > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "%s: m = %lld: must be below 2^31", who, (long long)m);
    GEMHIP_REQUIRE(st && ed, "%s: NULL pair arrays", who);
    const int64_t bad = first_bad_pair(st, ed, m, h->n);
    GEMHIP_REQUIRE(bad < 0, "%s: pair %lld = (%d,%d) outside [0,%lld)", who, (long long)bad, st[bad], ed[bad], (long long)h->n);
    return GEMHIP_OK;
}

int upload_pairs(gemhip_edgeclf *h, int64_t m, const int32_t *st, const int32_t *ed)
{
    GEMHIP_CHECK(h->st.upload(st, (size_t)m));
    GEMHIP_CHECK(h->ed.upload(ed, (size_t)m));
    h->last_m = m;
    return GEMHIP_OK;
}

// F [m][d] of the uploaded pairs into h->F; *ms_out the kernel's time.
int build_features(gemhip_edgeclf *h, int op, int64_t m, double *ms_out)
{
    GEMHIP_CHECK(h->F.reserve((size_t)m * h->d));
    GEMHIP_CHECK(start(h->watch));
    hipLaunchKernelGGL(ec_features_kernel, dim3(ec_grid(m)), dim3(EC_THREADS), 0, 0, h->X.get(), h->ld, h->d, op, h->st.get(), h->ed.get(), m, h->F.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(stop(h->watch, ms_out));
    return GEMHIP_OK;
}

struct NcOwner {                                             // destroys the solver's handle on every way out of gemhip_edgeclf_fit
    gemhip_nc_t h = nullptr;
    ~NcOwner() { if (h) gemhip_nc_destroy(h); }
};

}  // namespace

extern "C" int gemhip_edgeclf_create(int64_t n, int32_t d, int32_t ld, const float *X_host, gemhip_edgeclf_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "edgeclf_create: NULL output");
    *out = nullptr;
    const int rc = check_embedding("edgeclf_create", n, d, ld, X_host, 1, EC_MAX_D, "the solver's one LDS slab of padded rows");
    if (rc) return rc;
    const int64_t bad = first_bad_entry(X_host, n, d, ld, EC_MAX_ABS);
    if (bad >= 0) {
        const long long i = bad / d;
        const int c = (int)(bad % d);
        const float v = X_host[i * ld + c];
        GEMHIP_REQUIRE(std::isfinite(v), "edgeclf_create: X[%lld][%d] is not finite", i, c);
        return fail(GEMHIP_E_INVALID, "edgeclf_create: |X[%lld][%d]| = %g above %g (a pair feature could overflow fp32)", i, c, (double)std::fabs(v), (double)EC_MAX_ABS);
    }
    std::unique_ptr<gemhip_edgeclf> h(new gemhip_edgeclf);
    h->n = n; h->ld = ld; h->d = d;
    const double t0 = wall_ms();
    GEMHIP_CHECK(h->X.upload(X_host, (size_t)n * ld));
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->ms[0] = wall_ms() - t0;
    *out = h.release();
    return GEMHIP_OK;
}

extern "C" int gemhip_edgeclf_destroy(gemhip_edgeclf_t h)
{
    delete h;
    return GEMHIP_OK;
}

extern "C" int gemhip_edgeclf_features(gemhip_edgeclf_t h, int32_t op, int64_t m, const int32_t *st, const int32_t *ed, float *F_out)
{
    int rc = check_pairs("edgeclf_features", h, op, true, m, st, ed);
    if (rc) return rc;
    GEMHIP_REQUIRE(F_out != nullptr, "edgeclf_features: NULL output");
    if ((rc = upload_pairs(h, m, st, ed))) return rc;
    if ((rc = build_features(h, op, m, &h->ms[1]))) return rc;
    GEMHIP_CHECK(hipMemcpy(F_out, h->F, (size_t)m * h->d * sizeof(float), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_edgeclf_scores(gemhip_edgeclf_t h, int32_t op, int64_t m, const int32_t *st, const int32_t *ed, const double *w, double *score_out)
{
    int rc = check_pairs("edgeclf_scores", h, op, w != nullptr, m, st, ed);
    if (rc) return rc;
    GEMHIP_REQUIRE(score_out != nullptr, "edgeclf_scores: NULL output");
    if (w) {
        for (int j = 0; j < h->d; ++j) GEMHIP_REQUIRE(std::isfinite(w[j]), "edgeclf_scores: w[%d] is not finite", j);
        GEMHIP_REQUIRE(!std::isnan(w[h->d]), "edgeclf_scores: the intercept is NaN");
    }
    if ((rc = upload_pairs(h, m, st, ed))) return rc;
    if (w) GEMHIP_CHECK(h->w.upload(w, (size_t)h->d + 1));
    GEMHIP_CHECK(h->out.reserve((size_t)m));
    GEMHIP_CHECK(start(h->watch));
    hipLaunchKernelGGL(ec_scores_kernel, dim3(ec_grid(m)), dim3(EC_THREADS), 0, 0, h->X.get(), h->ld, h->d, w ? op : 0, h->st.get(), h->ed.get(), m,
                       w ? h->w.get() : (const double *)nullptr, h->out.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(stop(h->watch, &h->ms[2]));
    GEMHIP_CHECK(hipMemcpy(score_out, h->out, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_edgeclf_fit(gemhip_edgeclf_t h, int32_t op, int64_t m, const int32_t *st, const int32_t *ed, const uint8_t *label, double C, double dec_tol,
                                  int32_t max_iter, double *w_inout, double *info_out)
{
    int rc = check_pairs("edgeclf_fit", h, op, true, m, st, ed);
    if (rc) return rc;
    GEMHIP_REQUIRE(label != nullptr, "edgeclf_fit: NULL label");
    for (int64_t p = 0; p < m; ++p) GEMHIP_REQUIRE(label[p] <= 1, "edgeclf_fit: label[%lld] = %d is neither 0 nor 1", (long long)p, (int)label[p]);
    GEMHIP_REQUIRE(std::isfinite(C) && C > 0.0, "edgeclf_fit: C = %g (need a finite C > 0)", C);
    GEMHIP_REQUIRE(std::isfinite(dec_tol) && dec_tol > 0.0, "edgeclf_fit: dec_tol = %g (need a finite dec_tol > 0)", dec_tol);
    GEMHIP_REQUIRE(max_iter >= 1, "edgeclf_fit: max_iter = %d (need >= 1)", max_iter);
    GEMHIP_REQUIRE(w_inout != nullptr, "edgeclf_fit: NULL w");
    for (int j = 0; j <= h->d; ++j) GEMHIP_REQUIRE(std::isfinite(w_inout[j]), "edgeclf_fit: the start w[%d] is not finite", j);
    const double t0 = wall_ms();
    if ((rc = upload_pairs(h, m, st, ed))) return rc;
    if ((rc = build_features(h, op, m, &h->ms[5]))) return rc;
    NcOwner nc;
    rc = nc_create_from_device(m, h->d, h->d, h->F, &nc.h);
    h->F.reset();                                            // the solver has its copy
    if (rc) return rc;
    // one class, 0 = "is an edge": the CSR of the pairs' labels, every pair a training row
    std::vector<int64_t> row_ptr((size_t)m + 1);
    row_ptr[0] = 0;
    for (int64_t p = 0; p < m; ++p) row_ptr[p + 1] = row_ptr[p] + label[p];
    std::vector<int32_t> cls((size_t)row_ptr[m] + 1, 0), rows((size_t)m);
    for (int64_t p = 0; p < m; ++p) rows[p] = (int32_t)p;
    if ((rc = gemhip_nc_set_labels(nc.h, 1, row_ptr.data(), cls.data()))) return rc;
    double info[6] = {0, 0, 0, 0, 0, 0};
    if ((rc = gemhip_nc_fit(nc.h, m, rows.data(), C, dec_tol, max_iter, w_inout, info))) return rc;
    int64_t ninfo[8];
    double nms[4];
    if ((rc = gemhip_nc_info(nc.h, ninfo))) return rc;
    if ((rc = gemhip_nc_last_ms(nc.h, nms))) return rc;
    h->passes = ninfo[3]; h->loss_calls = ninfo[4]; h->iterations = ninfo[5];
    h->ms[3] = wall_ms() - t0;
    h->ms[4] = nms[2];
    if (info_out) {
        for (int q = 0; q < 6; ++q) info_out[q] = info[q];
        info_out[6] = (double)h->passes;
        info_out[7] = (double)h->loss_calls;
    }
    return GEMHIP_OK;
}

extern "C" int gemhip_edgeclf_last_ms(gemhip_edgeclf_t h, double *out)
{
    GEMHIP_REQUIRE(h && out, "edgeclf_last_ms: NULL");
    for (int q = 0; q < 6; ++q) out[q] = h->ms[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_edgeclf_info(gemhip_edgeclf_t h, int64_t *out)
{
    GEMHIP_REQUIRE(h && out, "edgeclf_info: NULL");
    out[0] = h->n; out[1] = h->d; out[2] = EC_PPW; out[3] = EC_PAIRS_PER_WG; out[4] = h->passes; out[5] = h->loss_calls; out[6] = h->iterations; out[7] = h->last_m;
    return GEMHIP_OK;
}
