// nc_host.hip -- node classification's host arithmetic (nc_host.hpp).  No HIP header, no device code: builds with a plain C++ compiler.
#include "nc_host.hpp"
#include <cmath>

namespace gemhip {

NcLabelError check_label_csr(int64_t n, int32_t K, const int64_t *row_ptr, const int32_t *cls)
{
    NcLabelError err;
    if (row_ptr[0] != 0) { err.kind = NcLabelError::ROW_PTR_FIRST; err.row = 0; return err; }
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) { err.kind = NcLabelError::ROW_PTR_DECREASES; err.row = i; return err; }
    if (row_ptr[n] != 0 && !cls) { err.kind = NcLabelError::CLS_NULL; return err; }
    std::vector<int64_t> seen_in((size_t)K, -1);          // the last row that listed the class
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int32_t c = cls[e];
            if (c < 0 || c >= K) { err.kind = NcLabelError::CLASS_OUT_OF_RANGE; err.row = i; err.index = e; err.cls = c; return err; }
            if (seen_in[c] == i) { err.kind = NcLabelError::CLASS_REPEATED; err.row = i; err.index = e; err.cls = c; return err; }
            seen_in[c] = i;
        }
    return err;
}

std::vector<int64_t> nc_class_positives(int32_t K, const int64_t *row_ptr, const int32_t *cls, int64_t n_train, const int32_t *train_idx)
{
    std::vector<int64_t> pos((size_t)K, 0);
    for (int64_t t = 0; t < n_train; ++t) {
        const int64_t i = train_idx[t];
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) ++pos[cls[e]];
    }
    return pos;
}

void nc_assemble(int d1, int dp, double C, const double *theta, double loss_sum, const double *gsum, const double *tiles, double *F_out, double *g_out,
                 double *H_out)
{
    const int d = d1 - 1, T = dp / 32;
    double w2 = 0.0;
    for (int j = 0; j < d; ++j) w2 += theta[j] * theta[j];
    *F_out = C * loss_sum + 0.5 * w2;
    for (int j = 0; j < d1; ++j) g_out[j] = C * gsum[j] + (j < d ? theta[j] : 0.0);
    int tile = 0;
    for (int ti = 0; ti < T; ++ti)
        for (int tj = ti; tj < T; ++tj, ++tile) {
            const double *t = tiles + (size_t)tile * 1024;
            for (int a = 0; a < 32; ++a) {
                const int i = ti * 32 + a;
                if (i >= d1) break;
                for (int b = 0; b < 32; ++b) {
                    const int j = tj * 32 + b;
                    if (j >= d1) break;
                    if (j < i) continue;                              // a diagonal tile: its upper half only
                    const double v = C * t[a * 32 + b] + (i == j && i < d ? 1.0 : 0.0);
                    H_out[(size_t)i * d1 + j] = v;
                    H_out[(size_t)j * d1 + i] = v;
                }
            }
        }
}

bool nc_newton_step(int d1, const double *H, const double *g, double *delta, double *dec, double *shift_out)
{
    *dec = 0.0;
    if (shift_out) *shift_out = 0.0;
    for (int j = 0; j < d1; ++j) delta[j] = 0.0;
    double dmax = 1.0;
    for (int i = 0; i < d1; ++i) {
        if (!std::isfinite(g[i])) return false;
        for (int j = i; j < d1; ++j)
            if (!std::isfinite(H[(size_t)i * d1 + j])) return false;
        dmax = std::fmax(dmax, std::fabs(H[(size_t)i * d1 + i]));
    }
    std::vector<double> L((size_t)d1 * d1), y((size_t)d1);
    double shift = 0.0;
    for (int attempt = 0; attempt <= NC_MAX_SHIFTS; ++attempt) {
        bool ok = true;
        for (int j = 0; j < d1 && ok; ++j) {                          // L L^T = H + shift I, column by column, L lower
            double s = H[(size_t)j * d1 + j] + shift;
            for (int k = 0; k < j; ++k) s -= L[(size_t)j * d1 + k] * L[(size_t)j * d1 + k];
            if (!(s > 0.0) || !std::isfinite(s)) { ok = false; break; }
            const double ljj = std::sqrt(s);
            L[(size_t)j * d1 + j] = ljj;
            for (int i = j + 1; i < d1; ++i) {
                double t = H[(size_t)j * d1 + i];                     // upper triangle: H[j][i], j < i
                for (int k = 0; k < j; ++k) t -= L[(size_t)i * d1 + k] * L[(size_t)j * d1 + k];
                L[(size_t)i * d1 + j] = t / ljj;
            }
        }
        if (ok) {
            for (int i = 0; i < d1; ++i) {                            // L y = -g
                double t = -g[i];
                for (int k = 0; k < i; ++k) t -= L[(size_t)i * d1 + k] * y[k];
                y[i] = t / L[(size_t)i * d1 + i];
            }
            for (int i = d1 - 1; i >= 0; --i) {                       // L^T delta = y
                double t = y[i];
                for (int k = i + 1; k < d1; ++k) t -= L[(size_t)k * d1 + i] * delta[k];
                delta[i] = t / L[(size_t)i * d1 + i];
            }
            double gd = 0.0;
            bool finite = true;
            for (int i = 0; i < d1; ++i) { gd += g[i] * delta[i]; finite = finite && std::isfinite(delta[i]); }
            if (finite) {
                *dec = -gd;
                if (shift_out) *shift_out = shift;
                return true;
            }
        }
        shift = shift == 0.0 ? 1e-10 * dmax : 10.0 * shift;
    }
    for (int j = 0; j < d1; ++j) delta[j] = 0.0;
    return false;
}

bool nc_begin_step(NcClass &c, int d1, double F, const double *g, const double *H)
{
    c.F = F;
    c.gmax = 0.0;
    for (int j = 0; j < d1; ++j) c.gmax = std::fmax(c.gmax, std::fabs(g[j]));
    c.delta.assign((size_t)d1, 0.0);
    c.alpha = 1.0;
    c.halvings = 0;
    if (!nc_newton_step(d1, H, g, c.delta.data(), &c.dec, &c.shift) || !(c.dec >= 0.0)) { c.stopped = true; return false; }
    return c.dec > NC_FULL_STEP_DEC * std::fmax(1.0, c.F);
}

void nc_trial_point(const NcClass &c, int d1, double *out)
{
    for (int j = 0; j < d1; ++j) out[j] = c.theta[j] + c.alpha * c.delta[j];
}

NcTrial nc_judge_trial(NcClass &c, double F_trial)
{
    if (std::isfinite(F_trial) && F_trial <= c.F - NC_ARMIJO_C1 * c.alpha * c.dec) return NC_ACCEPT;
    if (c.halvings >= NC_MAX_HALVINGS) { c.stopped = true; return NC_GIVE_UP; }
    c.alpha *= 0.5;
    ++c.halvings;
    ++c.backtracks;
    return NC_RETRY;
}

void nc_accept_step(NcClass &c, int d1, double dec_tol)
{
    for (int j = 0; j < d1; ++j) c.theta[j] += c.alpha * c.delta[j];
    ++c.iterations;
    if (c.dec <= dec_tol * std::fmax(1.0, c.F)) c.converged = true;
}

}  // namespace gemhip
