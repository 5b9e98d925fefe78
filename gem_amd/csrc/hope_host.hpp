// hope_host.hpp -- the host arithmetic of HOPE / Laplacian Eigenmaps / LLE (hope_host.hip): the fp64 small-matrix steps between the launches, the
// scheduling rules of the two solvers, the choice of the k outputs, the CSR set-up.  Plain C++, no HIP: everything here runs on a CPU
// (scripts/build_asan_hope_host.sh, tests/test_hope_host.py); the solvers (hope_solve.hip) launch and ask these functions what to do next; the entry points (hope.hip) word the refusals.
// Small matrices are row-major fp64 std::vectors unless a comment says otherwise.
#pragma once
#include <cstdint>
#include <vector>

namespace gemhip {

// ---------------------------------------------------------------- dense fp64 steps
// Upper-triangular Cholesky G = R^T R with a pivot floor; on success C = R^-1 (so that (Y C)^T (Y C) = I for G = Y^T Y).  False when a pivot
// falls to the floor or below (rank deficient or ill conditioned block): the caller then takes the rank-revealing eigen fallback.
bool chol_inverse(int b, const std::vector<double> &G, double floor, std::vector<double> &C);
// G <- D G D, D = diag(dinv), dinv[i] = 1 / sqrt(G_ii), or 0 where G_ii is not positive and finite (that diagonal entry becomes 0).  Returns dinv.
std::vector<double> normalise_gram(int b, std::vector<double> &G);
// Rank-revealing fallback: G = Z diag(w) Z^T (sym_eig; G is overwritten), the directions with w > rel * w_max, w > abs_floor and w > 0 are kept,
// C (b x nk) = Z[:, kept] / sqrt(w), largest first.  Returns nk (0: C is left alone).
int eig_fallback(int b, std::vector<double> &G, double rel, double abs_floor, std::vector<double> &C);
// The host half of one pass of orth() / orth_scaled(): from the Gram matrix of the block's `keep` columns to the keep x nk coefficients that
// orthonormalise it (Cholesky, else the fallback: *remixed = true, the columns are no longer triangular images of the input's).  Returns nk.
int orth_pass(int keep, std::vector<double> &G, double tol, double abs_floor, std::vector<double> &C, bool *remixed);
int orth_scaled_pass(int keep, std::vector<double> &G, std::vector<double> &C);
// M <- (M + M^T) / 2
void symmetrise(int n, std::vector<double> &M);
// The fused Rayleigh-Ritz projection: G2 = Y1^T Y1, H = Y1^T Op Y1  ->  C2 = chol(G2)^-1 (through the normalised G2) and H <- C2^T sym(H) C2.
// False (H as it was, C2 empty) when a column is null or a pivot is lost.
bool rr_project(int keep, std::vector<double> &G2, std::vector<double> &H, std::vector<double> &C2);
// The map of the eigen-path on an eigenvalue x.  kind 0: the Katz map beta x / (1 - beta x); 1: 1 + x; 2: beta - x.
double sym_f(int kind, double beta, double x);
// Ritz ordering: Z's columns (eigenvectors of the projected matrix, eigenvalues ev ascending) by |f(ev)| descending (stable) -> th, C = Z[:, order],
// C <- C2 C when C2 (upper triangular) is not empty, Ct = -C diag(th).
void ritz_order(int ma, const std::vector<double> &Z, const std::vector<double> &ev, int kind, double beta, const std::vector<double> &C2,
                std::vector<double> &th, std::vector<double> &C, std::vector<double> &Ct);

// ---------------------------------------------------------------- rules of the symmetric eigen-path
struct SymSpectrum { double L, smin, smax, res_floor; };       // |lambda| <= L, spectrum in [smin, smax]; residuals are relative to >= res_floor
SymSpectrum sym_spectrum(int kind, double beta, double br);
void sym_first_interval(int kind, double L, double &lo, double &hi);          // damp the unwanted three quarters
// One cycle's filter: centre c, half width e of the damped interval [lo, hi], in-filter deflation period q, degree m.
struct SymCycle { double c, e; int q, m; };
SymCycle sym_cycle_plan(double lo, double hi, double smin, double smax, const std::vector<double> &th, int nl, int cyc, double amp, double amp0,
                        int max_degree);
double sym_residual_scale(int want, const std::vector<double> &th, const std::vector<double> &res, double L, double res_floor);    // rmax
int sym_lock_count(int want, int b_min, const std::vector<double> &th, const std::vector<double> &res, double lock_tol, double res_floor);
// The next damped interval from the Ritz |f| in the middle of the oversampling columns (column jc, returned); tau_prev never falls.
int sym_next_interval(int kind, double beta, double L, int want_left, const std::vector<double> &th, double &tau_prev, double &lo, double &hi);

// ---------------------------------------------------------------- rules of the block-Krylov path
// basis capacity in columns; basis_cols_override: the value of GEMHIP_HOPE_BASIS_COLS, or null
int krylov_basis_capacity(int b, int krylov_steps, int64_t n, const int *basis_cols_override);
// Krylov steps of a cycle once nl pairs are locked; depth_cols_override: the value of GEMHIP_HOPE_DEPTH_COLS, or null
int krylov_steps_after_lock(int krylov_steps, int mmax, int nl, int m0, const int *depth_cols_override);
int krylov_b_min(int b, int oversample);
double lock_tolerance(float tol);                                               // both solvers
int krylov_lock_count(int want, int prev_b, int b_min, const std::vector<double> &act_sig, const std::vector<double> &D, double lock_tol);
// restart block: nb columns, C (ma x nb) = the leading Ritz vectors (Zt: column-major ma x mt).  Returns nb.
int krylov_restart_block(int mt, int b, int nl, int b_min, int ma, const std::vector<double> &Zt, std::vector<double> &C);

// ---------------------------------------------------------------- shared by both solvers
// sig = the k largest of `all`, descending; returns max |sig - sig_old| / sig[0] (0 if sig[0] <= 0) and sets sig_old = sig
double wanted_values(std::vector<double> all, int k, std::vector<double> &sig, std::vector<double> &sig_old);
// A candidate output: value s, sign of the left vector against the right one, basis column (>= nl with Zt given: active Ritz vector col - nl).
struct OutCand { double s, sgn; int col; };
// The k largest candidates (stable), placed by ASCENDING s: sigma[j] and column j of Cu, Cv ((nl + ma) x k).  from_image: the left vectors are
// taken from S V (scaled by 1 / s), not from V (scaled by sgn); unit_v: unit vectors out, not vectors times sqrt(s).  cand is left sorted.
void select_outputs(std::vector<OutCand> &cand, int k, int nl, int ma, const std::vector<double> *Zt, bool from_image, bool unit_v, float *sigma,
                    std::vector<double> &Cu, std::vector<double> &Cv);
// negate the output columns j of Cu, Cv (mc x k) with colmax[j] < 0; true if there was one
bool flip_negative_columns(int mc, int k, const std::vector<double> &colmax, std::vector<double> &Cu, std::vector<double> &Cv);
void fill_solve_stats(double *stats, double ms, double spmm_count, double spmm_cols, double terms, double basis, double cycles, double change, double br,
                      double residual, double spmm_ms);

// ---------------------------------------------------------------- knobs
// The fourteen GEMHIP_HOPE_* variables, read in one place.  Hope (hope_ops.hpp) holds one of these; it is filled when the state is made and again at
// the start of a plan set-up, a solve and an SVD-error estimate, so a variable set between two calls of a process is seen by the second.
struct HopeKnobs {
    int spmm16 = 1;                // _SPMM16: 0 = one row per wavefront, else 16 lanes per row up to 128 columns
    int spmm16_u = 0;              // _SPMM16_U: gathers in flight per row and round (>= 8, >= 4, else 2); <= 0 = by the block's width
    int colmax2 = 1;               // _COLMAX2: 0 = one block per column, else two coalesced passes
    int sym = -1;                  // _SYM: -1 = unset (the size rule of solve_operator decides), 0 = never the eigen-path, 1 = at any size
    double sym_amp = 1e4;          // _SYM_AMP, _SYM_AMP0: filter growth per cycle / of the first cycle, at least 10
    double sym_amp0 = 1e3;
    int sym_maxdeg = 32;           // _SYM_MAXDEG: filter degree per cycle, at least 2 (measured at SBM 100k/1M: 30-32 is cheapest, scripts/ab_hope_sym.py)
    bool sym_fused_rr = true;      // _SYM_FUSED_RR: off for a value that reads as 0
    bool no_lock = false;          // _NO_LOCK, _FIXED_DEPTH, _HOST_PROJECT, _DEBUG: on by presence, whatever the value
    bool fixed_depth = false;
    bool host_project = false;
    bool debug = false;
    bool has_basis_cols = false;   // _BASIS_COLS, _DEPTH_COLS: optional; the value goes to krylov_basis_capacity / krylov_steps_after_lock as it is
    bool has_depth_cols = false;
    int basis_cols = 0, depth_cols = 0;
    const int *basis_cols_override() const { return has_basis_cols ? &basis_cols : nullptr; }
    const int *depth_cols_override() const { return has_depth_cols ? &depth_cols : nullptr; }
};
// lookup(name): the variable's value or null -- getenv in the library, a table in the CPU tests
HopeKnobs hope_knobs_from_env(const char *(*lookup)(const char *));

// ---------------------------------------------------------------- set-up
enum class CsrError { NONE = 0, BAD_ARGUMENTS, ROW_PTR, COLUMN };
CsrError check_csr_arrays(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, int64_t *bad_edge);
// A^T by a stable counting sort: every row of A^T has its columns ascending
struct CsrT { std::vector<int64_t> rp; std::vector<int32_t> ci; std::vector<float> va; };
CsrT transpose_csr(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *va);
bool csr_is_symmetric(int64_t n, int64_t nnz, const int64_t *row_ptr, const CsrT &T);     // A == A^T entry for entry, T = transpose_csr(A)
double abs_sum_bound(int64_t n, const int64_t *row_ptr, const int32_t *col, const float *va);       // sqrt(max row sum x max column sum) >= sigma_max
int katz_terms(double br);                                                      // terms of the Katz series for beta rho(A) = br < 1
void lap_edge_values(int64_t n, const int64_t *row_ptr, const int32_t *col, const float *w, float *va);   // D^-1/2 A D^-1/2 (w null: ones)
void lle_edge_values(int64_t n, const int64_t *row_ptr, const float *w, float *va);                       // l1-normalised rows
void reverse_columns(float *V, int64_t n, int k);

}  // namespace gemhip
