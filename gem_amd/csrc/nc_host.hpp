// nc_host.hpp -- the host arithmetic of the node-classification handle (nc_host.hip): the label CSR check, the degenerate classes of a
// training set, the assembly of a class's objective from the pass kernel's sums, the Newton step and the line search's bookkeeping.
// Plain C++, no HIP: everything here runs on a CPU (scripts/build_asan_nc.sh, tests/test_node_classification.py); nc.hip words the refusals,
// uploads and launches.
//
// The objective of one class (sklearn LogisticRegression(penalty='l2', C, fit_intercept=True), the intercept unpenalised):
//     F(w, b) = C * sum_{i in T} log(1 + exp(-y_i (x_i . w + b))) + |w|^2 / 2,        theta = (w, b), d1 = d + 1 entries.
// Stopping rule (scale-free): a class is converged after the step whose Newton decrement lambda^2 = -g . delta satisfies
//     lambda^2 <= dec_tol * max(1, F).
// Line search: Armijo backtracking, c1 = 1e-4, halving from alpha = 1, at most NC_MAX_HALVINGS halvings (then the class stops as it is,
// unconverged).  A full step is taken WITHOUT evaluating the loss once lambda^2 <= NC_FULL_STEP_DEC * max(1, F): the Armijo difference
// c1 * lambda^2 (and the decrease lambda^2 / 2 a Newton step makes there) is then below the rounding of F itself, a sum of n fp64 terms
// whose error is a few hundred ulp of F at most, so a comparison of two such sums would decide nothing.
#pragma once
#include <cstdint>
#include <vector>

namespace gemhip {

constexpr double NC_ARMIJO_C1 = 1e-4;
constexpr double NC_FULL_STEP_DEC = 1e-13;       // relative to max(1, F): about 450 ulp of F
constexpr int NC_MAX_HALVINGS = 40;
constexpr int NC_MAX_SHIFTS = 60;

// What check_label_csr found wrong.  It never words a message: gemhip_nc_set_labels does.
struct NcLabelError {
    enum Kind { NONE = 0, ROW_PTR_FIRST, ROW_PTR_DECREASES, CLS_NULL, CLASS_OUT_OF_RANGE, CLASS_REPEATED } kind = NONE;
    int64_t row = -1;                  // the first offending row (ROW_PTR_DECREASES, CLASS_*)
    int64_t index = -1;                // the entry of cls (CLASS_*)
    int32_t cls = 0;                   // the class id found there
    explicit operator bool() const { return kind != NONE; }
};
// In this order, the first failure reported: row_ptr[0] == 0, no row of negative length, cls present when there are entries, every class id
// in [0, K), no class twice in a row (rows need not be sorted).  row_ptr has n + 1 entries.
NcLabelError check_label_csr(int64_t n, int32_t K, const int64_t *row_ptr, const int32_t *cls);

// pos[c] = how many of the training rows carry class c; a row listed twice counts twice.
std::vector<int64_t> nc_class_positives(int32_t K, const int64_t *row_ptr, const int32_t *cls, int64_t n_train, const int32_t *train_idx);
// -1: no positive among the training rows (b = -inf), +1: no negative (b = +inf), 0: both occur.
inline int nc_degenerate(int64_t positives, int64_t n_train) { return positives == 0 ? -1 : positives == n_train ? 1 : 0; }

// The objective, its gradient and its Hessian from the pass kernel's sums over the training rows, x~ = (x, 1):
//     F = C * loss_sum + |w|^2 / 2,   g = C * gsum + (w, 0),   H = C * sym(tiles) + diag(1, ..., 1, 0).
// tiles: the upper-triangle 32 x 32 tiles of X~^T diag(s) X~ in row-major tile order (0,0), (0,1), ..., (0,T-1), (1,1), ..., each [32][32] row
// major, T = dp / 32, dp = d1 rounded up to 32.  gsum has dp entries.  H_out [d1][d1] is filled symmetric from the upper triangle.
void nc_assemble(int d1, int dp, double C, const double *theta, double loss_sum, const double *gsum, const double *tiles, double *F_out, double *g_out,
                 double *H_out);

// Solves (H + shift I) delta = -g by Cholesky in fp64, reading the upper triangle of H [d1][d1].  shift = 0 unless a pivot is not positive;
// then (Levenberg) shift = 1e-10 * max(1, max |H_jj|) and ten times more per retry, at most NC_MAX_SHIFTS times.  *dec = -g . delta.
// Returns false (delta = 0, *dec = 0) if no shift made the matrix positive definite or H, g hold a non-finite value.
bool nc_newton_step(int d1, const double *H, const double *g, double *delta, double *dec, double *shift_out);

// One class of a fit.
struct NcClass {
    int32_t id = 0;
    int degenerate = 0;
    bool converged = false, stopped = false;          // stopped: the line search or the solve gave up; the class stays as it is
    int iterations = 0, backtracks = 0, halvings = 0;
    double F = 0.0, gmax = 0.0, dec = 0.0, alpha = 1.0, shift = 0.0;
    std::vector<double> theta, delta;                 // d1 each
};
enum NcTrial { NC_ACCEPT = 0, NC_RETRY = 1, NC_GIVE_UP = 2 };

// After a pass at c.theta: the step, its decrement, |g|_inf; alpha = 1.  Returns true if the step needs a loss evaluation (see above),
// false if it is to be accepted as it stands -- or if the solve failed (c.stopped).
bool nc_begin_step(NcClass &c, int d1, double F, const double *g, const double *H);
// theta + alpha * delta, the point the loss kernel evaluates.
void nc_trial_point(const NcClass &c, int d1, double *out);
// Armijo: F_trial <= F - c1 * alpha * lambda^2 accepts; otherwise alpha halves (one backtrack) until NC_MAX_HALVINGS.
NcTrial nc_judge_trial(NcClass &c, double F_trial);
// theta += alpha * delta, one iteration; converged if lambda^2 <= dec_tol * max(1, F).
void nc_accept_step(NcClass &c, int d1, double dec_tol);

}  // namespace gemhip
