// kmeans_host.hip -- k-means' host arithmetic (kmeans_host.hpp).  No HIP header, no device code: builds with a plain C++ compiler.
#include "kmeans_host.hpp"
#include <algorithm>
#include <cmath>
#include <limits>

namespace gemhip {

int64_t km_first_bad_uniform(const double *u, int64_t count)
{
    for (int64_t t = 0; t < count; ++t)
        if (!(u[t] >= 0.0 && u[t] < 1.0)) return t;
    return -1;
}

double km_mean_variance(const float *X, int64_t n, int32_t d, int64_t ld)
{
    std::vector<double> mean((size_t)d, 0.0), var((size_t)d, 0.0);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t c = 0; c < d; ++c) mean[c] += (double)X[i * ld + c];
    for (int32_t c = 0; c < d; ++c) mean[c] /= (double)n;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t c = 0; c < d; ++c) {
            const double t = (double)X[i * ld + c] - mean[c];
            var[c] += t * t;
        }
    double s = 0.0;
    for (int32_t c = 0; c < d; ++c) s += var[c] / (double)n;
    return s / (double)d;
}

void km_pad_centres(int32_t K, int32_t d, int32_t dpad, int32_t Kp, const float *C, float *Cp, float *cn)
{
    for (int32_t k = 0; k < Kp; ++k) {
        double s = 0.0;
        for (int32_t c = 0; c < dpad; ++c) {
            const float v = k < K && c < d ? C[(size_t)k * d + c] : 0.f;
            Cp[(size_t)k * dpad + c] = v;
            s += (double)v * (double)v;
        }
        cn[k] = k < K ? (float)s : std::numeric_limits<float>::infinity();
    }
}

void km_centres_from_sums(int32_t K, int32_t d, int32_t dpad, const double *sums, const int64_t *counts, float *C)
{
    for (int32_t k = 0; k < K; ++k)
        for (int32_t c = 0; c < d; ++c) C[(size_t)k * d + c] = counts[k] > 0 ? (float)(sums[(size_t)k * dpad + c] / (double)counts[k]) : 0.f;
}

double km_centre_shift(int32_t K, int32_t d, const float *a, const float *b)
{
    double s = 0.0;
    for (size_t q = 0; q < (size_t)K * d; ++q) {
        const double t = (double)a[q] - (double)b[q];
        s += t * t;
    }
    return s;
}

void km_relocation_order(int64_t n, const double *dist, int64_t n_take, int64_t *out)
{
    std::vector<int64_t> idx((size_t)n);
    for (int64_t i = 0; i < n; ++i) idx[i] = i;
    n_take = n_take < n ? n_take : n;
    std::partial_sort(idx.begin(), idx.begin() + n_take, idx.end(), [dist](int64_t a, int64_t b) { return dist[a] > dist[b] || (dist[a] == dist[b] && a < b); });
    for (int64_t j = 0; j < n_take; ++j) out[j] = idx[j];
}

int64_t km_relocate(int32_t K, int32_t dpad, const std::vector<int32_t> &empty, const int32_t *donor, const float *xrows, double *sums, int64_t *counts)
{
    (void)K;
    for (size_t j = 0; j < empty.size(); ++j) {
        const int32_t from = donor[j], to = empty[j];
        if (counts[from] <= 1) return (int64_t)j;
        for (int32_t c = 0; c < dpad; ++c) {
            const double x = (double)xrows[j * (size_t)dpad + c];
            sums[(size_t)from * dpad + c] -= x;
            sums[(size_t)to * dpad + c] = x;
        }
        counts[from] -= 1;
        counts[to] = 1;
    }
    return -1;
}

int64_t km_first_row(double u, int64_t n)
{
    const int64_t r = (int64_t)std::floor(u * (double)n);
    return r < 0 ? 0 : r < n ? r : n - 1;
}

int64_t km_find_block(const double *prefix, int64_t nb, double v)
{
    int64_t lo = 0, hi = nb;                                   // the first b in [0, nb) with prefix[b + 1] > v; prefix never decreases
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (prefix[mid + 1] > v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

int64_t km_find_in_block(double start, const float *vals, int64_t len, double v)
{
    double s = start;
    for (int64_t t = 0; t < len; ++t) {
        s += (double)vals[t];
        if (s > v) return t;
    }
    return -1;
}

namespace {

// -sum p log p of the positive counts; 0 when only one is positive (sklearn.metrics.cluster.entropy).
double count_entropy(const std::vector<int64_t> &m, double total)
{
    int positive = 0;
    for (int64_t v : m) positive += v > 0 ? 1 : 0;
    if (positive <= 1) return 0.0;
    double h = 0.0;
    for (int64_t v : m)
        if (v > 0) h -= ((double)v / total) * (std::log((double)v) - std::log(total));
    return h;
}

}  // namespace

bool km_scores(const int64_t *table, int32_t Kp, int32_t Kt, double *out)
{
    typedef unsigned __int128 u128;
    typedef __int128 i128;
    std::vector<int64_t> a((size_t)Kp, 0), b((size_t)Kt, 0);
    int64_t n = 0, majority = 0;
    u128 ss = 0;
    for (int32_t i = 0; i < Kp; ++i) {
        int64_t best = 0;
        for (int32_t j = 0; j < Kt; ++j) {
            const int64_t v = table[(size_t)i * Kt + j];
            if (v < 0) return false;
            a[i] += v; b[j] += v; n += v;
            ss += (u128)v * (u128)v;
            best = v > best ? v : best;
        }
        majority += best;
    }
    if (n < 1) return false;
    const double N = (double)n;
    int ra = 0, rb = 0;
    for (int64_t v : a) ra += v > 0 ? 1 : 0;
    for (int64_t v : b) rb += v > 0 ? 1 : 0;
    // ---- mutual information (sklearn.metrics.mutual_info_score, its terms and its clamps)
    double mi = 0.0;
    if (ra > 1 && rb > 1) {
        const double eps = std::numeric_limits<double>::epsilon();
        for (int32_t i = 0; i < Kp; ++i)
            for (int32_t j = 0; j < Kt; ++j) {
                const int64_t v = table[(size_t)i * Kt + j];
                if (v <= 0) continue;
                const double p = (double)v / N;
                const double term = p * (std::log((double)v) - std::log(N)) + p * (-std::log((double)a[i] * (double)b[j]) + std::log(N) + std::log(N));
                mi += std::fabs(term) < eps ? 0.0 : term;
            }
        mi = mi > 0.0 ? mi : 0.0;
    }
    const double h_pred = count_entropy(a, N), h_true = count_entropy(b, N);
    double nmi;
    if (ra == 1 && rb == 1) nmi = 1.0;
    else if (mi == 0.0) nmi = 0.0;
    else {
        const double norm = 0.5 * (h_true + h_pred);
        nmi = mi / (norm > std::numeric_limits<double>::epsilon() ? norm : std::numeric_limits<double>::epsilon());
    }
    // ---- adjusted Rand index (sklearn's pair-count form); n^2 at n = 2^31 and the products of two such counts stay below 2^127
    u128 sa = 0, sb = 0;
    for (int64_t v : a) sa += (u128)v * (u128)v;
    for (int64_t v : b) sb += (u128)v * (u128)v;
    const i128 tp = (i128)ss - (i128)n, fp = (i128)sa - (i128)ss, fn = (i128)sb - (i128)ss;
    const i128 tn = (i128)((u128)n * (u128)n) - fp - fn - (i128)ss;
    double ari;
    if (fp == 0 && fn == 0) ari = 1.0;
    else ari = 2.0 * (double)(tp * tn - fn * fp) / (double)((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn));
    out[0] = nmi;
    out[1] = ari;
    out[2] = (double)majority / N;
    out[3] = h_true > 0.0 ? mi / h_true : 1.0;
    return true;
}

}  // namespace gemhip
