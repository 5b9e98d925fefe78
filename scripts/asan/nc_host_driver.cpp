// Stand-alone AddressSanitizer / UBSan driver for node classification's host half (gem_amd/csrc/nc_host.hip), built and run by
// scripts/build_asan_nc.sh as plain C++ on a machine without a GPU.  It drives the label check through every refusal and a valid CSR, the
// degenerate-class detection, the assembly from upper-triangle tiles (d1 below, at and above a tile), the Cholesky and Levenberg paths of the
// Newton step, and the line search's bookkeeping on a one-dimensional logistic problem solved entirely on the host: accept, backtrack, the
// full step without a loss evaluation, convergence, and the give-up after NC_MAX_HALVINGS.
#include "../../gem_amd/csrc/nc_host.hpp"
#include <cmath>
#include <cstdio>
#include <vector>

using namespace gemhip;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static void labels()
{
    const int64_t rp_ok[] = {0, 2, 2, 3, 5};
    const int32_t cls_ok[] = {2, 0, 1, 0, 2};
    EXPECT(!check_label_csr(4, 3, rp_ok, cls_ok));
    const int64_t rp_first[] = {1, 2, 2, 3, 5};
    EXPECT(check_label_csr(4, 3, rp_first, cls_ok).kind == NcLabelError::ROW_PTR_FIRST);
    const int64_t rp_dec[] = {0, 2, 1, 3, 5};
    NcLabelError e = check_label_csr(4, 3, rp_dec, cls_ok);
    EXPECT(e.kind == NcLabelError::ROW_PTR_DECREASES && e.row == 1);
    EXPECT(check_label_csr(4, 3, rp_ok, nullptr).kind == NcLabelError::CLS_NULL);
    const int32_t cls_range[] = {2, 0, 3, 0, 2};
    e = check_label_csr(4, 3, rp_ok, cls_range);
    EXPECT(e.kind == NcLabelError::CLASS_OUT_OF_RANGE && e.index == 2 && e.row == 2 && e.cls == 3);
    const int32_t cls_twice[] = {2, 0, 1, 2, 2};
    e = check_label_csr(4, 3, rp_ok, cls_twice);
    EXPECT(e.kind == NcLabelError::CLASS_REPEATED && e.index == 4 && e.row == 3 && e.cls == 2);
    const int64_t rp_empty[] = {0, 0, 0};
    EXPECT(!check_label_csr(2, 1, rp_empty, nullptr));
    const int32_t train[] = {3, 0, 3, 1};                                    // row 3 twice
    const std::vector<int64_t> pos = nc_class_positives(3, rp_ok, cls_ok, 4, train);
    EXPECT(pos[0] == 3 && pos[1] == 0 && pos[2] == 3);
    EXPECT(nc_degenerate(pos[1], 4) == -1 && nc_degenerate(4, 4) == 1 && nc_degenerate(pos[0], 4) == 0);
}

static void assemble_and_solve()
{
    for (int d1 : {1, 2, 32, 33, 129}) {
        const int dp = (d1 + 31) & ~31, T = dp / 32, ntri = T * (T + 1) / 2;
        std::vector<double> tiles((size_t)ntri * 1024), theta((size_t)d1), gsum((size_t)dp), g((size_t)d1), H((size_t)d1 * d1), delta((size_t)d1);
        // tiles of M = A^T A + I for a deterministic A (positive definite), padded region poisoned
        std::vector<double> M((size_t)dp * dp, 1e300);
        for (int i = 0; i < d1; ++i)
            for (int j = 0; j < d1; ++j) {
                double s = i == j ? 1.0 : 0.0;
                for (int k = 0; k < 3; ++k) s += std::sin(1.0 + i * (k + 1)) * std::sin(1.0 + j * (k + 1));
                M[(size_t)i * dp + j] = s;
            }
        int tile = 0;
        for (int ti = 0; ti < T; ++ti)
            for (int tj = ti; tj < T; ++tj, ++tile)
                for (int a = 0; a < 32; ++a)
                    for (int b = 0; b < 32; ++b) tiles[(size_t)tile * 1024 + a * 32 + b] = M[(size_t)(ti * 32 + a) * dp + tj * 32 + b];
        for (int j = 0; j < d1; ++j) { theta[j] = 0.1 * j; gsum[j] = std::cos(j); }
        double F = 0.0;
        nc_assemble(d1, dp, 2.0, theta.data(), 3.0, gsum.data(), tiles.data(), &F, g.data(), H.data());
        double w2 = 0.0;
        for (int j = 0; j + 1 < d1; ++j) w2 += theta[j] * theta[j];
        EXPECT(std::fabs(F - (6.0 + 0.5 * w2)) < 1e-12);
        for (int i = 0; i < d1; ++i)
            for (int j = 0; j < d1; ++j) {
                EXPECT(H[(size_t)i * d1 + j] == H[(size_t)j * d1 + i]);
                const double want = 2.0 * M[(size_t)(i < j ? i : j) * dp + (i < j ? j : i)] + (i == j && i + 1 < d1 ? 1.0 : 0.0);
                EXPECT(std::fabs(H[(size_t)i * d1 + j] - want) < 1e-12);
            }
        double dec = 0.0, shift = -1.0;
        EXPECT(nc_newton_step(d1, H.data(), g.data(), delta.data(), &dec, &shift) && shift == 0.0 && dec > 0.0);
        double worst = 0.0;
        for (int i = 0; i < d1; ++i) {
            double r = g[i];
            for (int j = 0; j < d1; ++j) r += H[(size_t)i * d1 + j] * delta[j];
            worst = std::fmax(worst, std::fabs(r));
        }
        EXPECT(worst < 1e-9);
        // Levenberg: an indefinite matrix needs a shift; a NaN is refused
        std::vector<double> Hi = H;
        Hi[0] = -1.0;
        EXPECT(nc_newton_step(d1, Hi.data(), g.data(), delta.data(), &dec, &shift) && shift > 0.0 && dec >= 0.0);
        Hi[0] = std::nan("");
        EXPECT(!nc_newton_step(d1, Hi.data(), g.data(), delta.data(), &dec, nullptr) && dec == 0.0);
    }
}

// F(b) = sum log(1 + exp(-y (x w + b))) + w^2 / 2 on five points, d1 = 2
static void objective(const double *th, double *F, double *g, double *H)
{
    const double x[] = {-2.0, -1.0, 0.5, 1.0, 3.0};
    const int y[] = {0, 0, 1, 0, 1};
    *F = 0.5 * th[0] * th[0];
    if (g) { g[0] = th[0]; g[1] = 0.0; H[0] = 1.0; H[1] = H[2] = H[3] = 0.0; }
    for (int i = 0; i < 5; ++i) {
        const double z = x[i] * th[0] + th[1], p = 1.0 / (1.0 + std::exp(-z));
        *F += std::log1p(std::exp(-std::fabs(z))) + (y[i] ? std::fmax(-z, 0.0) : std::fmax(z, 0.0));
        if (g) {
            const double r = p - y[i], s = p * (1.0 - p);
            g[0] += x[i] * r; g[1] += r;
            H[0] += s * x[i] * x[i]; H[1] += s * x[i]; H[2] += s * x[i]; H[3] += s;
        }
    }
}

static void line_search()
{
    for (double start : {0.0, 40.0}) {                                       // from 40 the full Newton step overshoots: backtracks
        NcClass c;
        c.theta = {start, -start};
        int evaluations = 0;
        for (int it = 0; it < 60 && !c.converged && !c.stopped; ++it) {
            double F, g[2], H[4], trial[2], Ft;
            objective(c.theta.data(), &F, g, H);
            if (nc_begin_step(c, 2, F, g, H)) {
                for (;;) {
                    nc_trial_point(c, 2, trial);
                    objective(trial, &Ft, nullptr, nullptr);
                    ++evaluations;
                    const NcTrial v = nc_judge_trial(c, Ft);
                    if (v == NC_ACCEPT) { nc_accept_step(c, 2, 1e-10); break; }
                    if (v == NC_GIVE_UP) break;
                }
            } else if (!c.stopped)
                nc_accept_step(c, 2, 1e-10);
        }
        double F, g[2], H[4];
        objective(c.theta.data(), &F, g, H);
        EXPECT(c.converged && !c.stopped && std::fabs(g[0]) < 1e-6 && std::fabs(g[1]) < 1e-6 && evaluations > 0);
        EXPECT(start == 0.0 || c.backtracks > 0);
        std::printf("start %g: %d iterations, %d backtracks, %d loss evaluations, |g| = %.1e\n", start, c.iterations, c.backtracks, evaluations,
                    std::fmax(std::fabs(g[0]), std::fabs(g[1])));
    }
    NcClass c;                                                               // a trial that never decreases: gives up after NC_MAX_HALVINGS
    c.theta = {0.0, 0.0};
    const double g[2] = {1.0, 1.0}, H[4] = {1.0, 0.0, 0.0, 1.0};
    EXPECT(nc_begin_step(c, 2, 1.0, g, H));
    NcTrial v;
    int n = 0;
    while ((v = nc_judge_trial(c, std::nan(""))) == NC_RETRY) ++n;
    EXPECT(v == NC_GIVE_UP && n == NC_MAX_HALVINGS && c.stopped && c.backtracks == NC_MAX_HALVINGS);
    NcClass t;                                                               // a decrement below the loss's rounding: no evaluation asked for
    t.theta = {0.0, 0.0};
    const double gt[2] = {1e-9, 0.0};
    EXPECT(!nc_begin_step(t, 2, 5.0, gt, H) && !t.stopped);
    nc_accept_step(t, 2, 1e-10);
    EXPECT(t.converged && t.iterations == 1);
}

int main()
{
    labels();
    assemble_and_solve();
    line_search();
    std::printf("nc_host driver: %d failures\n", failures);
    return failures ? 1 : 0;
}
