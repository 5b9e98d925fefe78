// hope_host.hip -- the host arithmetic of HOPE / Laplacian Eigenmaps / LLE, moved out of hope.hip with its loops and the order of their
// floating-point operations as they were (interface and contracts: hope_host.hpp).  Plain C++ by the rule of sym_eig.hip: no HIP header, nothing
// from common.hpp, no kernel; the suffix only puts the file into the library's csrc/*.hip glob.
#include "hope_host.hpp"
#include "sym_eig.hpp"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

namespace gemhip {

// ------------------------------------------------------------------ dense fp64 steps
bool chol_inverse(int b, const std::vector<double> &G, double floor, std::vector<double> &C)
{
    std::vector<double> R((size_t)b * b, 0.0);
    for (int j = 0; j < b; ++j) {
        double djj = G[(size_t)j * b + j];
        for (int k = 0; k < j; ++k) djj -= R[(size_t)k * b + j] * R[(size_t)k * b + j];
        if (!(djj > floor)) return false;
        const double rjj = std::sqrt(djj);
        R[(size_t)j * b + j] = rjj;
        for (int i = j + 1; i < b; ++i) {
            double v = G[(size_t)j * b + i];
            for (int k = 0; k < j; ++k) v -= R[(size_t)k * b + j] * R[(size_t)k * b + i];
            R[(size_t)j * b + i] = v / rjj;
        }
    }
    C.assign((size_t)b * b, 0.0);                           // back substitution: R C = I, C upper triangular
    for (int j = 0; j < b; ++j) {
        C[(size_t)j * b + j] = 1.0 / R[(size_t)j * b + j];
        for (int i = j - 1; i >= 0; --i) {
            double v = 0.0;
            for (int k = i + 1; k <= j; ++k) v += R[(size_t)i * b + k] * C[(size_t)k * b + j];
            C[(size_t)i * b + j] = -v / R[(size_t)i * b + i];
        }
    }
    return true;
}

// (filtered columns differ in length by the filter's growth; an entry of the fp32 Gram matrix is accurate relative to the product of its two
// column norms, so the scaled matrix is accurate entrywise)
std::vector<double> normalise_gram(int b, std::vector<double> &G)
{
    std::vector<double> dinv(b, 0.0);
    for (int i = 0; i < b; ++i) { const double g = G[(size_t)i * b + i]; dinv[i] = (g > 0.0 && std::isfinite(g)) ? 1.0 / std::sqrt(g) : 0.0; }
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < b; ++j) G[(size_t)i * b + j] *= dinv[i] * dinv[j];
    for (int i = 0; i < b; ++i) if (dinv[i] == 0.0) G[(size_t)i * b + i] = 0.0;
    return dinv;
}

int eig_fallback(int b, std::vector<double> &G, double rel, double abs_floor, std::vector<double> &C)
{
    std::vector<double> w;
    sym_eig(b, G, w);                                         // ascending; G columns = eigenvectors
    const double lmax = std::max(w[b - 1], 0.0);
    int first = 0;
    while (first < b && !(w[first] > rel * lmax && w[first] > abs_floor && w[first] > 0.0)) ++first;
    const int nk = b - first;
    if (nk == 0) return 0;
    C.assign((size_t)b * nk, 0.0);
    for (int i = 0; i < b; ++i)
        for (int j = 0; j < nk; ++j) C[(size_t)i * nk + j] = G[(size_t)i * b + (b - 1 - j)] / std::sqrt(w[b - 1 - j]);
    return nk;
}

int orth_pass(int keep, std::vector<double> &G, double tol, double abs_floor, std::vector<double> &C, bool *remixed)
{
    double dmax = 0.0;
    for (int i = 0; i < keep; ++i) dmax = std::max(dmax, G[(size_t)i * keep + i]);
    // Cholesky pivots are Schur complements: a pivot below 1e-4 * dmax means condition > ~1e4 (or rank loss)
    if (chol_inverse(keep, G, std::max(1e-4 * dmax, abs_floor), C)) return keep;
    if (remixed) *remixed = true;
    return eig_fallback(keep, G, tol, abs_floor, C);
}

// CholeskyQR on the column-NORMALISED Gram matrix; the fallback drops directions below 1e-6 relative energy
int orth_scaled_pass(int keep, std::vector<double> &G, std::vector<double> &C)
{
    const std::vector<double> dinv = normalise_gram(keep, G);
    int nk = keep;
    if (!chol_inverse(keep, G, 1e-5, C)) nk = eig_fallback(keep, G, 1e-6, 0.0, C);
    for (int i = 0; i < keep && nk > 0; ++i)
        for (int j = 0; j < nk; ++j) C[(size_t)i * nk + j] *= dinv[i];
    return nk;
}

void symmetrise(int n, std::vector<double> &M)
{
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) { const double v = 0.5 * (M[(size_t)i * n + j] + M[(size_t)j * n + i]); M[(size_t)i * n + j] = M[(size_t)j * n + i] = v; }
}

bool rr_project(int keep, std::vector<double> &G2, std::vector<double> &H, std::vector<double> &C2)
{
    const std::vector<double> dinv = normalise_gram(keep, G2);
    C2.clear();
    for (int i = 0; i < keep; ++i) if (dinv[i] == 0.0) return false;
    if (!chol_inverse(keep, G2, 1e-5, C2)) { C2.clear(); return false; }
    for (int i = 0; i < keep; ++i)
        for (int j = 0; j < keep; ++j) C2[(size_t)i * keep + j] *= dinv[i];
    symmetrise(keep, H);                                    // Hq = C2^T sym(H1) C2 (C2 upper triangular)
    std::vector<double> T((size_t)keep * keep, 0.0), Hq((size_t)keep * keep, 0.0);
    for (int i = 0; i < keep; ++i)                          // T = H1 C2
        for (int l = 0; l < keep; ++l) {
            const double h = H[(size_t)i * keep + l];
            if (h == 0.0) continue;
            for (int j = l; j < keep; ++j) T[(size_t)i * keep + j] += h * C2[(size_t)l * keep + j];
        }
    for (int l = 0; l < keep; ++l)                          // Hq = C2^T T
        for (int i = l; i < keep; ++i) {
            const double c = C2[(size_t)l * keep + i];
            if (c == 0.0) continue;
            for (int j = 0; j < keep; ++j) Hq[(size_t)i * keep + j] += c * T[(size_t)l * keep + j];
        }
    H.swap(Hq);
    return true;
}

double sym_f(int kind, double beta, double x) { return kind == 1 ? 1.0 + x : kind == 2 ? beta - x : beta * x / (1.0 - beta * x); }

void ritz_order(int ma, const std::vector<double> &Z, const std::vector<double> &ev, int kind, double beta, const std::vector<double> &C2,
                std::vector<double> &th, std::vector<double> &C, std::vector<double> &Ct)
{
    std::vector<int> order(ma);
    for (int j = 0; j < ma; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return std::fabs(sym_f(kind, beta, ev[x])) > std::fabs(sym_f(kind, beta, ev[y])); });
    th.assign(ma, 0.0);
    C.assign((size_t)ma * ma, 0.0); Ct.assign((size_t)ma * ma, 0.0);
    for (int j = 0; j < ma; ++j) {
        th[j] = ev[order[j]];
        for (int i = 0; i < ma; ++i) C[(size_t)i * ma + j] = Z[(size_t)i * ma + order[j]];
    }
    if (!C2.empty()) {                                      // the block is Y1, not Q = Y1 C2: its coefficients are C2 W
        std::vector<double> M((size_t)ma * ma, 0.0);
        for (int i = 0; i < ma; ++i)
            for (int l = i; l < ma; ++l) {
                const double c = C2[(size_t)i * ma + l];
                if (c == 0.0) continue;
                for (int j = 0; j < ma; ++j) M[(size_t)i * ma + j] += c * C[(size_t)l * ma + j];
            }
        C.swap(M);
    }
    for (int j = 0; j < ma; ++j)
        for (int i = 0; i < ma; ++i) Ct[(size_t)i * ma + j] = -th[j] * C[(size_t)i * ma + j];
}

// ------------------------------------------------------------------ rules of the symmetric eigen-path
SymSpectrum sym_spectrum(int kind, double beta, double br)
{
    const double L = kind == 1 ? 1.0001 : kind == 2 ? beta : br / std::fabs(beta);   // |lambda| <= L: power-iteration estimate + margin
    return {L, kind == 2 ? 0.0 : -L, L, kind == 2 ? 0.25 * L : 0.0};                // (LLE's wanted eigenvalues start at 0: residuals relative to the scale)
}

void sym_first_interval(int kind, double L, double &lo, double &hi) { lo = kind == 2 ? 0.25 * L : -L; hi = kind == 2 ? L : 0.5 * L; }

SymCycle sym_cycle_plan(double lo, double hi, double smin, double smax, const std::vector<double> &th, int nl, int cyc, double amp, double amp0,
                        int max_degree)
{
    const double c = 0.5 * (hi + lo), e = 0.5 * (hi - lo);
    const double tmax = std::max(smax - c, c - smin) / e;
    const double rho = tmax + std::sqrt(std::max(tmax * tmax - 1.0, 0.0));
    // in-filter deflation period: edge growth <= 1e6 between projections (numpy mirror, SBM 100k/1M: 1e3 / 1e4 / 1e5 / 1e6 give the
    // same singular values with 50 / 34 / 26 / 16 projections per solve; at 1e8 the error grows tenfold.  On the device: 1e5 -> 1e6 takes a
    // solve from 15.6 to 14.65 ms with all 64 sigma still inside the ARPACK bar, 1e7 is no faster, 1e8 fails tests/test_hope_gpu.py)
    const int q = (int)std::max(1.0, std::floor(std::log(1e6) / std::log(std::max(rho, 1.0001))));
    double rho_m = rho;                                       // growth that caps the degree: the spectrum's edge, or -- once pairs are
    if (nl > 0 && cyc > 0 && !th.empty()) {                   // locked and deflated inside the filter -- the largest active Ritz value
        double ta = 1.0;
        for (double t : th) ta = std::max(ta, 1.02 * std::fabs(t - c) / e);
        ta = std::min(ta, tmax);
        rho_m = ta + std::sqrt(std::max(ta * ta - 1.0, 0.0));
    }
    const int m = (int)std::max(2.0, std::min((double)max_degree, std::floor(std::log(cyc == 0 ? amp0 : amp) / std::log(std::max(rho_m, 1.0001)))));
    return {c, e, q, m};
}

double sym_residual_scale(int want, const std::vector<double> &th, const std::vector<double> &res, double L, double res_floor)
{
    double rmax = 0.0;
    for (int j = 0; j < std::min(want, (int)th.size()); ++j) rmax = std::max(rmax, res[j] / std::max(std::max(std::fabs(th[j]), 1e-3 * L), res_floor));
    return rmax;
}

int sym_lock_count(int want, int b_min, const std::vector<double> &th, const std::vector<double> &res, double lock_tol, double res_floor)
{
    const int ma = (int)th.size();
    int newl = 0;
    while (newl < want - 1 && newl < ma - b_min && res[newl] < lock_tol * std::max(std::fabs(th[newl]), res_floor)) ++newl;
    return newl;
}

// bounded where |f| is below the Ritz |f| in the MIDDLE of the oversampling columns (th is sorted by |f|): the j-th Ritz |f| never exceeds
// the j-th true one, so no wanted value is damped, and straggling last columns cannot hold the cut-off down.  Never lowered.
int sym_next_interval(int kind, double beta, double L, int want_left, const std::vector<double> &th, double &tau_prev, double &lo, double &hi)
{
    const int ma = (int)th.size();
    const int jc = std::max(0, std::min(ma - 1, want_left + (ma - want_left) / 2 - 1));
    const double tau = std::max(tau_prev, std::fabs(sym_f(kind, beta, th[jc])));
    tau_prev = tau;
    if (!(tau > 0.0)) sym_first_interval(kind, L, lo, hi);
    else if (kind == 2) { lo = std::max(beta - tau, 0.01 * L); hi = L; }
    else if (kind == 1) { hi = std::min(tau - 1.0, 0.98 * L); lo = -L; if (hi < -0.5 * L) hi = -0.5 * L; }
    else {
        hi = std::min(tau / (std::fabs(beta) * (1.0 + tau)), 0.98 * L);
        lo = -std::min(L, tau < 1.0 ? tau / (std::fabs(beta) * (1.0 - tau)) : L);
        if (lo > -1e-6 * L) lo = -1e-6 * L;
    }
    return jc;
}

// ------------------------------------------------------------------ rules of the block-Krylov path
// (krylov_steps + 1) blocks for the first cycles, 20 % more for the deeper polynomial of the locked phase (fewer cycles and SpMMs against a
// dearer projected eigenproblem: measured optimum, scripts/hope_basis_sweep.sh); at most n and 512
int krylov_basis_capacity(int b, int krylov_steps, int64_t n, const int *basis_cols_override)
{
    int64_t basis_cols = (int64_t)b * (krylov_steps + 1);
    basis_cols += basis_cols / 5;
    if (basis_cols_override) basis_cols = std::max<int64_t>((int64_t)b * (krylov_steps + 1), *basis_cols_override);
    return (int)std::min<int64_t>(std::min<int64_t>(basis_cols, n), 512);
}

// the basis budget (mmax columns) that locked pairs no longer need buys a deeper Krylov polynomial for the rest
int krylov_steps_after_lock(int krylov_steps, int mmax, int nl, int m0, const int *depth_cols_override)
{
    if (!(nl > 0 && m0 > 0)) return krylov_steps;
    const int cols = depth_cols_override ? std::min(mmax, std::max(*depth_cols_override, nl + m0)) : mmax;
    return std::max(krylov_steps, (cols - nl) / m0 - 1);
}

int krylov_b_min(int b, int oversample) { return std::min(b, std::max(2 * oversample, 16)); }

// (|sigma error| / sigma ~ residual^2 * sigma^2 / gap, so sqrt(tol) / 10 keeps locked values inside `tol`)
double lock_tolerance(float tol) { return 0.1 * std::sqrt(std::max((double)tol, 1e-12)); }

int krylov_lock_count(int want, int prev_b, int b_min, const std::vector<double> &act_sig, const std::vector<double> &D, double lock_tol)
{
    int newl = 0;
    while (newl < want - 1 && newl < prev_b - b_min && act_sig[newl] > 0 &&
           std::sqrt(std::max(D[(size_t)newl * prev_b + newl], 0.0)) < lock_tol * act_sig[newl] * act_sig[newl]) ++newl;
    return newl;
}

int krylov_restart_block(int mt, int b, int nl, int b_min, int ma, const std::vector<double> &Zt, std::vector<double> &C)
{
    const int nb = std::min(mt, std::max(b - nl, b_min));
    C.assign((size_t)ma * nb, 0.0);
    for (int i = 0; i < ma; ++i)
        for (int j = 0; j < nb; ++j) C[(size_t)i * nb + j] = Zt[(size_t)j * ma + i];
    return nb;
}

// ------------------------------------------------------------------ shared by both solvers
double wanted_values(std::vector<double> all, int k, std::vector<double> &sig, std::vector<double> &sig_old)
{
    std::sort(all.begin(), all.end(), std::greater<double>());
    for (int j = 0; j < k; ++j) sig[j] = all[j];
    double change = 0.0;
    for (int j = 0; j < k; ++j) change = std::max(change, std::fabs(sig[j] - sig_old[j]));
    sig_old = sig;
    return sig[0] > 0 ? change / sig[0] : 0.0;
}

void select_outputs(std::vector<OutCand> &cand, int k, int nl, int ma, const std::vector<double> *Zt, bool from_image, bool unit_v, float *sigma,
                    std::vector<double> &Cu, std::vector<double> &Cv)
{
    std::stable_sort(cand.begin(), cand.end(), [](const OutCand &x, const OutCand &y) { return x.s > y.s; });
    Cu.assign((size_t)(nl + ma) * k, 0.0); Cv.assign((size_t)(nl + ma) * k, 0.0);
    for (int r = 0; r < k; ++r) {
        const int j = k - 1 - r, col = cand[r].col;         // output column (ascending sigma: svds order, hope.py:33)
        const double s = cand[r].s;
        sigma[j] = (float)s;
        const double su = !from_image ? cand[r].sgn * std::sqrt(s) : unit_v ? (s > 0 ? 1.0 / s : 0.0) : (s > 0 ? 1.0 / std::sqrt(s) : 0.0);
        const double sv = unit_v ? 1.0 : std::sqrt(s);
        if (!Zt || col < nl) { Cu[(size_t)col * k + j] = su; Cv[(size_t)col * k + j] = sv; }
        else
            for (int i = 0; i < ma; ++i) {
                const double wv = (*Zt)[(size_t)(col - nl) * ma + i];
                Cu[(size_t)(nl + i) * k + j] = wv * su; Cv[(size_t)(nl + i) * k + j] = wv * sv;
            }
    }
}

bool flip_negative_columns(int mc, int k, const std::vector<double> &colmax, std::vector<double> &Cu, std::vector<double> &Cv)
{
    bool any = false;
    for (int j = 0; j < k; ++j)
        if (colmax[j] < 0) {
            any = true;
            for (int i = 0; i < mc; ++i) { Cu[(size_t)i * k + j] = -Cu[(size_t)i * k + j]; Cv[(size_t)i * k + j] = -Cv[(size_t)i * k + j]; }
        }
    return any;
}

void fill_solve_stats(double *stats, double ms, double spmm_count, double spmm_cols, double terms, double basis, double cycles, double change, double br,
                      double residual, double spmm_ms)
{
    stats[0] = ms * 1e-3; stats[1] = spmm_count; stats[2] = spmm_cols; stats[3] = terms; stats[4] = basis; stats[5] = cycles;
    stats[6] = change; stats[7] = br; stats[8] = eig_seconds(); stats[9] = eig_calls(); stats[10] = residual; stats[11] = spmm_ms * 1e-3;
}

// ------------------------------------------------------------------ set-up
HopeKnobs hope_knobs_from_env(const char *(*lookup)(const char *))
{
    HopeKnobs kn;
    if (const char *e = lookup("GEMHIP_HOPE_SPMM16")) kn.spmm16 = atoi(e);
    if (const char *e = lookup("GEMHIP_HOPE_SPMM16_U")) kn.spmm16_u = atoi(e);
    if (const char *e = lookup("GEMHIP_HOPE_COLMAX2")) kn.colmax2 = atoi(e);
    if (const char *e = lookup("GEMHIP_HOPE_SYM")) kn.sym = atoi(e) != 0;
    if (const char *e = lookup("GEMHIP_HOPE_SYM_AMP")) kn.sym_amp = std::max(10.0, atof(e));
    if (const char *e = lookup("GEMHIP_HOPE_SYM_AMP0")) kn.sym_amp0 = std::max(10.0, atof(e));
    if (const char *e = lookup("GEMHIP_HOPE_SYM_MAXDEG")) kn.sym_maxdeg = std::max(2, atoi(e));
    if (const char *e = lookup("GEMHIP_HOPE_SYM_FUSED_RR")) kn.sym_fused_rr = atoi(e) != 0;
    kn.no_lock = lookup("GEMHIP_HOPE_NO_LOCK") != nullptr;
    kn.fixed_depth = lookup("GEMHIP_HOPE_FIXED_DEPTH") != nullptr;
    kn.host_project = lookup("GEMHIP_HOPE_HOST_PROJECT") != nullptr;
    kn.debug = lookup("GEMHIP_HOPE_DEBUG") != nullptr;
    if (const char *e = lookup("GEMHIP_HOPE_BASIS_COLS")) { kn.has_basis_cols = true; kn.basis_cols = atoi(e); }
    if (const char *e = lookup("GEMHIP_HOPE_DEPTH_COLS")) { kn.has_depth_cols = true; kn.depth_cols = atoi(e); }
    return kn;
}

CsrError check_csr_arrays(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, int64_t *bad_edge)
{
    if (!(n >= 2 && nnz >= 0 && row_ptr && (nnz == 0 || col))) return CsrError::BAD_ARGUMENTS;
    if (!(row_ptr[0] == 0 && row_ptr[n] == nnz)) return CsrError::ROW_PTR;
    for (int64_t e = 0; e < nnz; ++e)
        if (!(col[e] >= 0 && col[e] < n)) { if (bad_edge) *bad_edge = e; return CsrError::COLUMN; }
    return CsrError::NONE;
}

CsrT transpose_csr(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *va)
{
    CsrT T;
    T.rp.assign(n + 1, 0); T.ci.resize(std::max<int64_t>(nnz, 1)); T.va.resize(std::max<int64_t>(nnz, 1));
    for (int64_t e = 0; e < nnz; ++e) ++T.rp[col[e] + 1];
    for (int64_t i = 0; i < n; ++i) T.rp[i + 1] += T.rp[i];
    std::vector<int64_t> at(T.rp.begin(), T.rp.end() - 1);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) { const int64_t q = at[col[e]]++; T.ci[q] = (int32_t)i; T.va[q] = va[e]; }
    return T;
}

// Transposing A^T gives A with every row's columns ascending (stable counting sort), which is how A^T itself is stored: equal arrays => the
// matrices are equal (duplicates, if any, are summed by the SpMM on both sides alike).
bool csr_is_symmetric(int64_t n, int64_t nnz, const int64_t *row_ptr, const CsrT &T)
{
    if (!(nnz > 0 && std::memcmp(T.rp.data(), row_ptr, (size_t)(n + 1) * sizeof(int64_t)) == 0)) return false;
    std::vector<int64_t> at(row_ptr, row_ptr + n);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t e = T.rp[j]; e < T.rp[j + 1]; ++e) {          // entry (j, i) of A^T = entry (i, j) of A: goes to row i, next free slot
            const int64_t i = T.ci[e], qpos = at[i]++;
            if (T.ci[qpos] != (int32_t)j || T.va[qpos] != T.va[e]) return false;
        }
    return true;
}

double abs_sum_bound(int64_t n, const int64_t *row_ptr, const int32_t *col, const float *va)
{
    double rs_max = 0.0, cs_max = 0.0;
    std::vector<double> cs(n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        double rs = 0.0;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) { rs += std::fabs(va[e]); cs[col[e]] += std::fabs(va[e]); }
        rs_max = std::max(rs_max, rs);
    }
    for (int64_t i = 0; i < n; ++i) cs_max = std::max(cs_max, cs[i]);
    return std::sqrt(rs_max * cs_max);
}

int katz_terms(double br)
{
    const int terms = (br <= 0.0) ? 0 : (int)std::ceil(std::log(1e-8) / std::log(br));
    return std::max(1, std::min(terms, 400));
}

void lap_edge_values(int64_t n, const int64_t *row_ptr, const int32_t *col, const float *w, float *va)
{
    std::vector<double> dinv(n, 0.0);
    for (int64_t i = 0; i < n; ++i) {
        double deg = 0.0;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) deg += w ? w[e] : 1.0;
        // zero-degree nodes: D^-1/2 = 0, so in T = I + M they sit at 1 (eigenvalue 1 of L_sym, not the 0 of networkx's all-zero row).  That is what the
        // reference's ARPACK call returns -- zero rows at these nodes -- while every wanted eigenvalue is below 1 (tests/README_lap_lle.md)
        dinv[i] = deg > 0.0 ? 1.0 / std::sqrt(deg) : 0.0;
    }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) va[e] = (float)(dinv[i] * (w ? w[e] : 1.0) * dinv[col[e]]);
}

void lle_edge_values(int64_t n, const int64_t *row_ptr, const float *w, float *va)
{
    for (int64_t i = 0; i < n; ++i) {
        double l1 = 0.0;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) l1 += std::fabs(w ? w[e] : 1.0);
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) va[e] = l1 > 0.0 ? (float)((w ? w[e] : 1.0) / l1) : 0.f;   // sklearn normalize(norm='l1')
    }
}

// the solvers return their k columns by ascending sigma; Laplacian Eigenmaps and LLE hand them out the other way round
void reverse_columns(float *V, int64_t n, int k)
{
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < k / 2; ++j) std::swap(V[i * k + j], V[i * k + (k - 1 - j)]);
}

}  // namespace gemhip
