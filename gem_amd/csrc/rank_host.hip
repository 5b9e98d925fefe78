// rank_host.hip -- the device-free half of the binary ranking metrics: see rank_host.hpp.  Plain C++ in a .hip file so that the library's
// build picks it up; scripts/build_asan_rank.sh compiles it as C++ under ASan / UBSan.
#include "rank_host.hpp"
#include <cmath>

namespace gemhip {

int64_t rank_first_nan(const double *score, int64_t m)
{
    for (int64_t t = 0; t < m; ++t)
        if (std::isnan(score[t])) return t;
    return -1;
}

int64_t rank_first_bad_label(const uint8_t *label, int64_t m)
{
    for (int64_t t = 0; t < m; ++t)
        if (label[t] > 1) return t;
    return -1;
}

int rank_active_passes(const uint32_t *hist, int64_t m, bool *active)
{
    int n_active = 0;
    for (int p = 0; p < RANK_PASSES; ++p) {
        bool one_bucket = false;
        for (int b = 0; b < RANK_BUCKETS; ++b) one_bucket = one_bucket || (int64_t)hist[p * RANK_BUCKETS + b] == m;
        active[p] = !one_bucket;
        n_active += active[p] ? 1 : 0;
    }
    return n_active;
}

RankGroupError rank_from_groups(int64_t T, const int64_t *tp, const int64_t *fp, double *out, int64_t *counts, int64_t *bad_group)
{
    if (T < 1) return RANK_EMPTY;
    int64_t ptp = 0, pfp = 0;
    for (int64_t g = 0; g < T; ++g) {
        const bool grows = tp[g] >= ptp && fp[g] >= pfp && (tp[g] > ptp || fp[g] > pfp);
        if (!grows || tp[g] > INT32_MAX || fp[g] > INT32_MAX || tp[g] + fp[g] > INT32_MAX) {
            if (bad_group) *bad_group = g;
            return RANK_NOT_CUMULATIVE;
        }
        ptp = tp[g]; pfp = fp[g];
    }
    const int64_t P = ptp, N = pfp;
    if (P == 0) return RANK_NO_POSITIVE;
    if (N == 0) return RANK_NO_NEGATIVE;
    int64_t U2 = 0;
    double ap = 0.0;
    ptp = 0; pfp = 0;
    for (int64_t g = 0; g < T; ++g) {
        const int64_t pos = tp[g] - ptp, neg = fp[g] - pfp;
        U2 += rank_u2_term(pos, neg, fp[g], N);
        ap += rank_ap_term(pos, tp[g], fp[g]);
        ptp = tp[g]; pfp = fp[g];
    }
    out[0] = (double)U2 / (double)(2 * P * N);                  // both integers are exact in fp64 below 2^53: then the quotient is correctly rounded
    out[1] = ap / (double)P;
    out[2] = (double)P / (double)(P + N);
    out[3] = 0.0;
    counts[0] = P; counts[1] = N; counts[2] = T; counts[3] = U2;
    return RANK_OK;
}

}  // namespace gemhip
