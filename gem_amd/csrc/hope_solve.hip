// hope_solve.hip -- the two solvers behind HOPE, Laplacian Eigenmaps and LLE: the restarted block-Krylov SVD (krylov_svd), the Chebyshev-filtered
// subspace iteration for symmetric operators (sym_filter_svd), the output step and the statistics they share, and solve_operator, which picks one.
// No kernel here: every launch goes through hope_ops.hpp, every host step between two launches through hope_host.hpp; the GEMHIP_HOPE_* variables
// arrive as H.knobs.
#include "hope_ops.hpp"
#include "sym_eig.hpp"
#include <chrono>

using namespace gemhip;

// orth, orth_scaled and cheb_filter are declared in hope_ops.hpp: the solvers below call them, and so do their test hooks (hope_hooks.hip).
namespace gemhip {

// Orthonormalise the b columns of Y (n x b, ld) in place (Tmp = scratch).  Well-conditioned blocks take a
// CholeskyQR step (Y <- Y R^-1); otherwise the Gram eigen-decomposition Y <- Y W L^-1/2 drops directions whose
// relative energy is below `tol` or whose absolute energy is below `abs_floor` (rank revealing: orth_pass).  Two passes.
int orth(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, double tol, double abs_floor, int passes, bool *remixed)
{
    return orth_passes(H, Y, ld, b, Tmp, ldt, passes, [&](int keep, std::vector<double> &G, std::vector<double> &C) {
        const int nk = orth_pass(keep, G, tol, abs_floor, C, remixed);
        tol = 1e-12; abs_floor = 0.0;                          // second pass only polishes
        return nk;
    });
}

}  // namespace gemhip

namespace {

// ------------------------------------------------------------------- what both solvers end with
// The compact [n][k] block Tmp goes to the caller's n x k output
void copy_out(Hope &H, const float *Tmp, int k, float *dst)
{
    HOPE_TRY(H, hipMemcpy(dst, Tmp, (size_t)H.n * k * sizeof(float), hipMemcpyDefault /* host (gemhip_hope_plan_solve) or device (.._solve_device) destination */));
}

// dst (n x k) = basis[:, :mc] C: one tall-skinny GEMM into Tmp, then the copy out
void emit(Hope &H, const float *basis, int ld, int mc, const std::vector<double> &C, int k, float *Tmp, float *dst)
{
    tsgemm(H, basis, ld, mc, C, k, 1.0f, nullptr, 0, Tmp, k);
    copy_out(H, Tmp, k, dst);
}

// Closes the solve's device window and its SpMM timers and fills stats[] (the arguments from `terms` on: fill_solve_stats).  Returns the window in ms.
float finish_solve(Hope &H, SolveEvents &tm, double *stats, double terms, double basis, double cycles, double change, double br, double residual)
{
    double window = 0.0;
    if (!H.err) { (void)tm.mark(1, H.s); (void)tm.ms(0, 1, &window); }
    const float ms = (float)window;
    if (!H.err) spmm_time_collect(H); else H.sp_used = 0;
    if (stats && !H.err) fill_solve_stats(stats, ms, H.spmm_count, H.spmm_cols, terms, basis, cycles, change, br, residual, H.spmm_ms);
    return ms;
}

// ------------------------------------------------------------------- block-Krylov path
// Restarted block-Krylov SVD of the operator the Hope state encodes (H.mode).  out_mode 0: U sqrt(S), V sqrt(S) (HOPE);
// out_mode 1: unit right singular vectors only (symmetric operators: eigenvectors).  sigma ascending.
int krylov_svd(Hope &H, int64_t n, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed,
                      int terms, double br, int out_mode, float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats)
{
    const int b = (int)std::min<int64_t>((int64_t)k + oversample, n);
    const HopeKnobs &kn = H.knobs;
    const int mmax = krylov_basis_capacity(b, krylov_steps, n, kn.basis_cols_override());
    GEMHIP_REQUIRE(b <= 512 && k <= mmax, "hope: k + oversample = %d too large (max 512)", b);
    const int ldm = (mmax + 31) / 32 * 32, ldb = (b + 31) / 32 * 32;
    DevBuf<float> Vall, Ball, T0, T1, W0, Tmp;
    auto dalloc = [&](DevBuf<float> &p, size_t cols) { HOPE_TRY(H, p.reserve((size_t)n * cols)); HOPE_TRY(H, hipMemset(p, 0, (size_t)n * cols * sizeof(float))); };
    dalloc(Vall, ldm); dalloc(Ball, ldm); dalloc(T0, ldb); dalloc(T1, ldb); dalloc(W0, ldb); dalloc(Tmp, ldm);
    SolveEvents tm;                 // (declared after the buffers: destroyed before they are freed, on every way out)
    if (tm.create(H, stats != nullptr)) return H.err;
    (void)tm.mark(0, H.s);

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
    const bool locking = !kn.no_lock;
    const double lock_tol = lock_tolerance(tol);
    const int b_min = krylov_b_min(b, oversample);
    double last_change = 1.0, last_residual = 1.0;
    bool exact = false;
    const bool debug = kn.debug;
    for (int rs = 0; rs <= max_restarts && !H.err; ++rs) {
        mc = nl + m0;
        int prev_off = nl, prev_b = m0, b_valid = nl;               // Ball columns [0, b_valid) hold S Vall
        const int steps = kn.fixed_depth ? krylov_steps : krylov_steps_after_lock(krylov_steps, mmax, nl, m0, kn.depth_cols_override());
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
            auto project = [&](int cols) {
                if (!kn.host_project) { project_out(H, Vall, ldm, mc, Wp, ldb, cols); return; }
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
        // the left vectors if the caller takes them, else the right ones: the first output, and the block the signs are read from
        const float *first = U_sqrtS ? Ball.get() : Vall.get();
        std::vector<double> &Cfirst = U_sqrtS ? Cu : Cv;
        float *dst_first = U_sqrtS ? U_sqrtS : V_sqrtS;
        tsgemm(H, first, ldm, mc, Cfirst, k, 1.0f, nullptr, 0, Tmp, k);           // compact [n][k]
        std::vector<float> cm(k, 0.f);
        if (!H.err) {
            colmax(H, Tmp, k, k, d_cm);
            HOPE_TRY(H, hipMemcpyAsync(cm.data(), d_cm, (size_t)k * sizeof(float), hipMemcpyDeviceToHost, H.s));
            HOPE_TRY(H, hipStreamSynchronize(H.s));
        }
        if (flip_negative_columns(mc, k, std::vector<double>(cm.begin(), cm.end()), Cu, Cv)) emit(H, first, ldm, mc, Cfirst, k, Tmp, dst_first);
        else copy_out(H, Tmp, k, dst_first);                                      // no sign flipped: the product stands
        if (U_sqrtS) emit(H, Vall, ldm, mc, Cv, k, Tmp, V_sqrtS);
    }
    finish_solve(H, tm, stats, terms, mc, restarts_done, last_change, br, last_residual);
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

}  // namespace

namespace gemhip {

// CholeskyQR on the column-NORMALISED Gram matrix, with the scaled Gram's eigen-decomposition as the fallback (orth_scaled_pass)
int orth_scaled(Hope &H, float *Y, int ld, int b, float *Tmp, int ldt, int passes)
{
    return orth_passes(H, Y, ld, b, Tmp, ldt, passes, [](int keep, std::vector<double> &G, std::vector<double> &C) { return orth_scaled_pass(keep, G, C); });
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

}  // namespace gemhip

namespace {

// Returns H.err; *fell_back = true when the iteration broke down or did not converge in max_cycles (the caller then runs the
// general block-Krylov solver); outputs are only written on success.
// kind 0: the Katz map f(x) = beta x / (1 - beta x) (HOPE; two-sided, outputs U sqrt(s), V sqrt(s));  kind 1: f(x) = 1 + x on the
// normalised adjacency D^-1/2 A D^-1/2, spectrum in [-1, 1] (Laplacian Eigenmaps: the largest eigenvalues of I + M; one-sided, outputs
// unit eigenvectors and f);  kind 2: f(x) = c - x on N^T N, N = I - P, spectrum in [0, c], c = H.beta (LLE: the SMALLEST eigenvalues;
// one-sided at the lower end, two SpMMs per application, outputs unit eigenvectors and f).
int sym_filter_svd(Hope &H, int kind, int64_t n, int32_t k, int32_t oversample, int32_t max_cycles, float tol, uint64_t seed, double br,
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
    const bool debug = H.knobs.debug, fused_rr = H.knobs.sym_fused_rr;
    const double amp = H.knobs.sym_amp, amp0 = H.knobs.sym_amp0;
    const int max_degree = H.knobs.sym_maxdeg;
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
    (void)tm.mark(0, H.s);
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
        if (U_sqrtS) emit(H, Vall, ldv, mc, Cu, k, Tmp, U_sqrtS);
        emit(H, Vall, ldv, mc, Cv, k, Tmp, V_sqrtS);
        // (measured: forming both outputs first and copying them out from two host threads side by side is 0.3 ms SLOWER per solve)
    }
    const auto ht3 = std::chrono::steady_clock::now();
    // stats[3]: no Katz series, f on the eigenvalues (-1: the Laplacian-Eigenmaps map, -2: LLE)
    const float ms = finish_solve(H, tm, stats, kind >= 1 ? -(double)kind : 0.0, nl + ma, cycles, last_change, br, last_residual);
    if (debug) {
        auto us = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b2) { return std::chrono::duration<double, std::micro>(b2 - a).count(); };
        fprintf(stderr, "[hope-sym] host timeline (us): set-up %.0f | cycles %.0f | outputs %.0f | final event and spmm timers %.0f ; device window %.0f\n",
                us(ht0, ht1), us(ht1, ht2), us(ht2, ht3), us(ht3, std::chrono::steady_clock::now()), ms * 1e3);
    }
    return H.err;
}

}  // namespace

namespace gemhip {

// One solve of the operator H holds (H.mode), with fresh statistics.  Symmetric operators (`symmetric`: always for Laplacian Eigenmaps and LLE;
// HOPE passes A == A^T and beta > 0 -- undirected graphs: every GEM example and the SBM benchmark) take the Chebyshev-filtered eigen-path:
// GEMHIP_HOPE_SYM=0 disables it, =1 takes it at any size; by default graphs under 16384 nodes stay on the block-Krylov solver (already milliseconds
// there).  If the eigen-path does not converge: the general solver, statistics reset again.  terms, br, out_mode: see krylov_svd.
int solve_operator(Hope &H, bool symmetric, int32_t k, int32_t oversample, int32_t krylov_steps, int32_t max_restarts, float tol, uint64_t seed,
                   int terms, double br, int out_mode, float *U_sqrtS, float *V_sqrtS, float *sigma, double *stats)
{
    reset_solve_stats(H);
    refresh_knobs(H);
    const bool sym_ok = symmetric && (int64_t)k + oversample + 1 < H.n;
    if (sym_ok && (H.knobs.sym >= 0 ? H.knobs.sym != 0 : (H.n >= 16384 && 8 * ((int64_t)k + oversample) <= H.n))) {
        bool fell_back = false;
        const int rc = sym_filter_svd(H, H.mode, H.n, k, oversample, std::max(40, 3 * (int)max_restarts), tol, seed, br, U_sqrtS, V_sqrtS, sigma, stats, &fell_back);
        if (rc || !fell_back) return rc;
        reset_solve_stats(H);
    }
    return krylov_svd(H, H.n, k, oversample, krylov_steps, max_restarts, tol, seed, terms, br, out_mode, U_sqrtS, V_sqrtS, sigma, stats);
}

}  // namespace gemhip
