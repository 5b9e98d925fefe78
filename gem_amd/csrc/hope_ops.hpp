// hope_ops.hpp -- the device operations of HOPE / Laplacian Eigenmaps / LLE (hope_ops.hip): the solver state, one launch function per operation,
// the operator applications made of them, and the two templates that take a host step as a callable.  hope_solve.hip (the two solvers), hope.hip
// (plans and entry points) and hope_hooks.hip (building blocks and test hooks) call these and hold no kernel.  What the host does between the
// launches is in hope_host.hpp.
#pragma once
#include "common.hpp"
#include "hope_host.hpp"
#include <algorithm>
#include <cmath>
#include <vector>

namespace gemhip {

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
    HopeKnobs knobs;                                         // the GEMHIP_HOPE_* variables as of the last refresh_knobs(); the hooks overwrite kernel variants
    int last_spmm_c = 0, last_spmm_u = 0;                    // the instantiation spmm() launched last: <CPL16, U>, or <CPL> with U = 0 (the hooks report it)
    int err = 0;
    Hope();          // knobs from the environment
    ~Hope()          // the events; the buffers free themselves
    {
        for (hipEvent_t e : sp_pool) hipEventDestroy(e);
        for (CoefSlot &c : coef) if (c.done) hipEventDestroy(c.done);
    }
};

#define HOPE_TRY(h, x) do { if (!(h).err) { hipError_t _e = (x); if (_e != hipSuccess) { (h).err = fail(GEMHIP_E_HIP, "hope: %s: %s", #x, hipGetErrorString(_e)); } } } while (0)

// H.knobs <- the process environment now.  The one place the HOPE units read it: Hope's constructor, and the start of a plan set-up (hope_setup), a
// solve (solve_operator) and an SVD-error estimate (svd_error_impl).  No launch function reads the environment.
void refresh_knobs(Hope &H);

// ---------------------------------------------------------------------- launch functions (hope_ops.hip; contracts at the definitions)
void spmm(Hope &H, bool transpose, float alpha, const float *X, int ldx, const float *Wadd, int ldw, float *Y, int ldy, int b,
          float wa = 1.0f, const float *W2 = nullptr, int ldw2 = 0, float wb = 0.f);
void gram_launch(Hope &H, const float *X, int ldx, int m1, const float *Y, int ldy, int m2, float *Gf, bool second = false);
void gram(Hope &H, const float *X, int ldx, int m1, const float *Y, int ldy, int m2, std::vector<double> &Gh);
void gram2(Hope &H, const float *Xa, int ldxa, int ma1, const float *Ya, int ldya, int ma2, std::vector<double> &Ga,
           const float *Xb, int ldxb, int mb1, const float *Yb, int ldyb, int mb2, std::vector<double> &Gb);
void tsgemm(Hope &H, const float *X, int ldx, int m, const std::vector<double> &Ch, int b2, float alpha, const float *Src, int lds_, float *Out, int ldo);
void ritz_rotate(Hope &H, const float *V, int ldv, const float *B, int ldb, int m, const std::vector<double> &Ch, const std::vector<double> &theta, int b2,
                 float *Out, int ldo, std::vector<double> &res2);
void colmax(Hope &H, const float *X, int ld, int mc, float *val);
void project_out(Hope &H, const float *V, int ldv, int m, float *W, int ldw, int cols);
void lincomb(Hope &H, int b, float a, const float *X, int ldx, float b2, const float *Y, int ldy, float c, const float *Z, int ldz, float *Out, int ldo);
void randn(Hope &H, float *X, int b, int ld, uint64_t seed);
void apply_S(Hope &H, const float *X, int ldx, int b, int terms, float *T0, float *T1, float *W0, int ldt, float *Out, int ldo);
void apply_ST(Hope &H, const float *Y, int ldy, int b, int terms, float *T0, float *T1, int ldt, float *Out, int ldo);
void apply_sym_op(Hope &H, int kind, float alpha, const float *X, int ldx, int cols, float *T, int ldt, float *Out, int ldo, float wa, const float *W,
                  int ldw, float wb, const float *W2, int ldw2);
int upload_csr(Hope &H, const char *who, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *va, const CsrT *T);
void upload_csr_w(Hope &H, int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, bool with_transpose);
void spmm_time_collect(Hope &H);
void reset_solve_stats(Hope &H);

// ---------------------------------------------------------------------- the solvers (hope_solve.hip)
int solve_operator(Hope &H, bool symmetric, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed,
                   int terms, double br, int out_mode, float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats);

// The solvers' own compositions, shared with their test hooks (definitions and contracts in hope_solve.hip)
int orth(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, double tol, double abs_floor = 0.0, int passes = 2, bool *remixed = nullptr);
int orth_scaled(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, int passes);
void cheb_filter(Hope &H, int kind, float *V, int ldv, int cols, int m, double c, double e, float *const F[3], int ldf, float *Ts, const float *Q, int ldq,
                 int nl, int q);

// ---------------------------------------------------------------------- the set-up estimates (hope.hip), shared with their test hook
// Both run power_iteration (below) on the operator H holds (A and A^T uploaded) and apply the margin the set-up relies on.
double katz_rho_estimate(Hope &H, const int64_t *row_ptr, const int32_t *col, const float *va);     // >= sigma_max(A): hope_setup's rho, margin and cap applied
double lle_shift_estimate(Hope &H);                                                                   // >= sigma_max(I - P)^2: gemhip_lle's c (H holds P, P^T)

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

// ---------------------------------------------------------------------- timing
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
// The two marks around a solve (device window, stats[0]).  create() also arms the SpMM timers.
struct SolveEvents : EventMarks<2> {
    int create(Hope &H, bool time_spmm)
    {
        if (!H.err) { HOPE_TRY(H, EventMarks<2>::create()); H.time_spmm = time_spmm; }
        return H.err;
    }
};

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

}  // namespace gemhip
