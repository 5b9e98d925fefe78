// hope.hip -- the entry points of HOPE (Katz-proximity truncated SVD), Laplacian Eigenmaps and LLE for MI355X (gfx950): the HOPE plan and its
// solves, the one-shot forms, the SVD-error estimator, gemhip_lap_eigmap and gemhip_lle.  Each sets its operator up (CSR checks, edge values,
// uploads, a spectral bound) and hands it to solve_operator (hope_solve.hip); the kernels and their launch functions are in hope_ops.hip, the host
// arithmetic in hope_host.hip, the building-block exports and test hooks in hope_hooks.hip.
#include "hope_ops.hpp"
#include <memory>

using namespace gemhip;

// The CSR checks of gemhip_hope_plan_create, gemhip_lap_eigmap and gemhip_lle; `who` is the entry point's message prefix.  Host reads only: it
// runs before the entry point's first HIP call, so a bad graph is GEMHIP_E_INVALID on a machine without a GPU too.
static int check_csr(const char *who, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col)
{
    int64_t e = 0;
    const CsrError err = check_csr_arrays(n, nnz, row_ptr, col, &e);
    GEMHIP_REQUIRE(err != CsrError::BAD_ARGUMENTS, "%s: bad CSR arguments", who);
    GEMHIP_REQUIRE(err != CsrError::ROW_PTR, "%s: row_ptr inconsistent with nnz", who);
    GEMHIP_REQUIRE(err != CsrError::COLUMN, "%s: column %d outside [0,%lld)", who, col[e], (long long)n);
    return GEMHIP_OK;
}

struct gemhip_hope_plan {
    Hope H;
    int terms = 1;
    double br = 0.0;
    bool symmetric = false;                          // A == A^T entry for entry (columns sorted within rows): the eigen-path applies
    double frob2_A = 0.0;                            // sum of the squared edge weights: ||beta A||_F^2 = beta^2 x this (gemhip_hope_plan_svd_error)
};

// ------------------------------------------------------------------ the two spectrum estimates of the set-ups
namespace gemhip {

// sigma_max(A) >= rho(A) by power iteration on A^T A (at most 40 steps; the 10 % margin covers what the stopping rule leaves); the max absolute
// row / column sums bound it too.  H holds A and A^T; row_ptr, col, va: the same A on the host.  Errors are in H.err.
double katz_rho_estimate(Hope &H, const int64_t *row_ptr, const int32_t *col, const float *va)
{
    const double rho = std::sqrt(power_iteration(H, 0.37, 12.9898, 40, 4, 1e-3, true, [&](float *X2, float *y) {
        spmm(H, false, 1.0f, X2, 2, nullptr, 0, y, 1, 1);                            // y = A x
        spmm(H, true, 1.0f, y, 1, nullptr, 0, X2 + 1, 2, 1);                         // z = A^T y
    }));
    return std::min(std::max(rho * 1.1, 1e-30), abs_sum_bound(H.n, row_ptr, col, va));
}

// c >= sigma_max(I - P)^2 by power iteration on N^T N (at most 60 steps), with a 5 % margin.  H holds P and P^T.  Errors are in H.err.
double lle_shift_estimate(Hope &H)
{
    const double est = power_iteration(H, 0.61, 7.31, 60, 8, 1e-4, false, [&](float *X2, float *t) {
        apply_sym_op(H, 2, 1.0f, X2, 2, 1, t, 1, X2 + 1, 2, 1.0f, nullptr, 0, 0.f, nullptr, 0);            // z = N^T N x
    });
    return est > 0.0 ? est * 1.05 : 4.0;
}

}  // namespace gemhip

// Graph-dependent setup of the Katz operator: A and A^T in CSR on the device, number of series terms from sigma_max(A).
static int hope_setup(gemhip_hope_plan &P, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta)
{
    if (const int rc = check_csr("hope", n, nnz, row_ptr, col)) return rc;
    Hope &H = P.H;
    refresh_knobs(H);
    H.beta = beta;
    std::vector<float> va(std::max<int64_t>(nnz, 1));                    // values default to 1
    for (int64_t e = 0; e < nnz; ++e) { va[e] = w ? w[e] : 1.0f; P.frob2_A += (double)va[e] * (double)va[e]; }
    const CsrT T = transpose_csr(n, nnz, row_ptr, col, va.data());
    P.symmetric = csr_is_symmetric(n, nnz, row_ptr, T);
    if (upload_csr(H, "hope", n, nnz, row_ptr, col, va.data(), &T)) return H.err;
    const double rho = katz_rho_estimate(H, row_ptr, col, va.data());
    if (H.err) return H.err;
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

// The plan of a one-shot entry point: destroyed on every way out
struct PlanDestroy { void operator()(gemhip_hope_plan *P) const { gemhip_hope_plan_destroy(P); } };
typedef std::unique_ptr<gemhip_hope_plan, PlanDestroy> OwnedPlan;
static int create_owned(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, OwnedPlan &out)
{
    gemhip_hope_plan_t P = nullptr;
    const int rc = gemhip_hope_plan_create(n, nnz, row_ptr, col, w, beta, &P);
    out.reset(P);
    return rc;
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
// 1.9 ms of a 13.5 ms solve at n = 100k, k = 64.  The solvers' output copy (hope_solve.hip: copy_out) uses hipMemcpyDefault, so this is the same code path.
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
    OwnedPlan P;
    if (const int rc = create_owned(n, nnz, row_ptr, col, w, beta, P)) return rc;
    // gemhip_last_call_phases: the plan (transpose, symmetry test, uploads, spectral-radius estimate) counts as host preparation as a whole;
    // kernel_seconds = the solver's own figure (stats[0]: device work and the projected host eigensolves between them), the rest of the solve
    // call is the two n x k outputs reaching the caller's pageable buffers
    const double t_solve = phase_now();
    phase_acc()[PH_HOST] = t_solve - t_call;
    double st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int rc = gemhip_hope_plan_solve(P.get(), k, oversample, krylov_steps, max_restarts, tol, seed, U_sqrtS, V_sqrtS, sigma, st);
    if (stats) for (int q = 0; q < 12; ++q) stats[q] = st[q];
    const double t_done = phase_now();
    phase_acc()[PH_KERNELS] = st[0];
    phase_acc()[PH_D2H] = std::max(0.0, (t_done - t_solve) - st[0]);
    P.reset();                                       // (the total includes freeing the plan, as it always has)
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
    refresh_knobs(H);
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
    OwnedPlan P;
    if (const int rc = create_owned(n, nnz, row_ptr, col, w, beta, P)) return rc;
    return gemhip_hope_plan_svd_error_uv(P.get(), k, sigma, U_sqrtS, V_sqrtS, probes, seed, err_out, frob2_out, uside_out);
}

// One-shot form for the plugin's verbose mode (hope.py:38-40): the plan is rebuilt (transpose + uploads), which costs about as much as the estimate itself.
extern "C" int gemhip_hope_svd_error(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, float beta, int32_t k,
                                     const float *sigma, const float *V_sqrtS, int32_t probes, uint64_t seed, double *err_out, double *frob2_out)
{
    OwnedPlan P;
    if (const int rc = create_owned(n, nnz, row_ptr, col, w, beta, P)) return rc;
    return gemhip_hope_plan_svd_error(P.get(), k, sigma, V_sqrtS, probes, seed, err_out, frob2_out);
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
    const double c = lle_shift_estimate(H);
    if (H.err) return H.err;
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

