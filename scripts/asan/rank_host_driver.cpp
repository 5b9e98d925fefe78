// Stand-alone driver of gem_amd/csrc/rank_host.hip for scripts/build_asan_rank.sh: every host function on small built cases, the results
// checked against values worked out by hand or by a quadratic count.  Plain C++, its own main; prints one summary line, exits non-zero on a
// wrong value.
#include "../../gem_amd/csrc/rank_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

using namespace gemhip;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- keys: ascending key = descending score, the zeros tied, the round trip
    {
        const double order[] = {inf, 1e308, 2.0, 1.0 + 2.220446049250313e-16, 1.0, 4.9e-324, 0.0, -4.9e-324, -1.0, -1e308, -inf};
        const int n = (int)(sizeof(order) / sizeof(order[0]));
        for (int i = 0; i + 1 < n; ++i) EXPECT(rank_key(order[i]) < rank_key(order[i + 1]));
        EXPECT(rank_key(0.0) == rank_key(-0.0));
        EXPECT(rank_key(inf) == 0x000fffffffffffffull && rank_key(-inf) == 0xfff0000000000000ull);
        for (int i = 0; i < n; ++i) EXPECT(rank_score_of_key(rank_key(order[i])) == order[i]);
        EXPECT(!std::signbit(rank_score_of_key(rank_key(-0.0))));
    }
    // ---- checks
    {
        const double s[5] = {0.5, inf, -inf, nan, nan};
        EXPECT(rank_first_nan(s, 3) == -1 && rank_first_nan(s, 5) == 3 && rank_first_nan(s, 0) == -1);
        const uint8_t y[4] = {0, 1, 1, 2};
        EXPECT(rank_first_bad_label(y, 3) == -1 && rank_first_bad_label(y, 4) == 3);
    }
    // ---- which passes move something
    {
        const double s[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
        std::vector<uint32_t> hist((size_t)RANK_PASSES * RANK_BUCKETS, 0);
        auto count = [&](const double *v, int m) {
            std::fill(hist.begin(), hist.end(), 0u);
            for (int i = 0; i < m; ++i)
                for (int p = 0; p < RANK_PASSES; ++p) ++hist[(size_t)p * RANK_BUCKETS + ((rank_key(v[i]) >> (8 * p)) & 255)];
        };
        bool active[RANK_PASSES];
        count(s, 6);
        EXPECT(rank_active_passes(hist.data(), 6, active) == 0);
        const double t[3] = {1.0, 1.0 + 2.220446049250313e-16, 1.0};                        // the lowest byte alone differs
        count(t, 3);
        EXPECT(rank_active_passes(hist.data(), 3, active) == 1 && active[0] && !active[7]);
        const double u[2] = {1.0, -1.0};                                                     // every byte differs between the signs
        count(u, 2);
        EXPECT(rank_active_passes(hist.data(), 2, active) == RANK_PASSES);
    }
    // ---- metrics from a group table against a quadratic count
    {
        // scores 3 3 2 2 2 1 0 0, labels 1 0 1 1 0 0 1 0
        const int64_t tp[4] = {1, 3, 3, 4}, fp[4] = {1, 2, 3, 4};
        double out[4];
        int64_t counts[4], bad = -1;
        EXPECT(rank_from_groups(4, tp, fp, out, counts, &bad) == RANK_OK);
        const double sc[8] = {3, 3, 2, 2, 2, 1, 0, 0};
        const int lab[8] = {1, 0, 1, 1, 0, 0, 1, 0};
        int64_t u2 = 0;
        for (int i = 0; i < 8; ++i)
            for (int j = 0; j < 8; ++j)
                if (lab[i] && !lab[j]) u2 += sc[i] > sc[j] ? 2 : sc[i] == sc[j] ? 1 : 0;
        EXPECT(counts[0] == 4 && counts[1] == 4 && counts[2] == 4 && counts[3] == u2);
        EXPECT(out[0] == (double)u2 / 32.0);
        const double ap = (1.0 * (1.0 / 2.0) + 2.0 * (3.0 / 5.0) + 0.0 + 1.0 * (4.0 / 8.0)) / 4.0;
        EXPECT(std::fabs(out[1] - ap) < 1e-15 && out[2] == 0.5 && out[3] == 0.0);
        const int64_t one_tp[1] = {5}, one_fp[1] = {7};                                      // all tied
        EXPECT(rank_from_groups(1, one_tp, one_fp, out, counts, &bad) == RANK_OK && out[0] == 0.5 && std::fabs(out[1] - 5.0 / 12.0) < 1e-16);
        const int64_t big_tp[2] = {1073741823, 1073741823}, big_fp[2] = {0, 1073741824};     // m = 2^31 - 1: U2 = 2 P N fits
        EXPECT(rank_from_groups(2, big_tp, big_fp, out, counts, &bad) == RANK_OK && out[0] == 1.0 && counts[3] == 2 * big_tp[1] * big_fp[1]);
    }
    // ---- refusals
    {
        double out[4];
        int64_t counts[4], bad = -1;
        const int64_t a[2] = {1, 1}, b[2] = {1, 1};
        EXPECT(rank_from_groups(0, a, b, out, counts, &bad) == RANK_EMPTY);
        EXPECT(rank_from_groups(2, a, b, out, counts, &bad) == RANK_NOT_CUMULATIVE && bad == 1);
        const int64_t c[2] = {2, 1}, d[2] = {0, 3};
        EXPECT(rank_from_groups(2, c, d, out, counts, &bad) == RANK_NOT_CUMULATIVE && bad == 1);
        const int64_t z[2] = {0, 0}, g[2] = {1, 2};
        EXPECT(rank_from_groups(2, z, g, out, counts, &bad) == RANK_NO_POSITIVE && rank_from_groups(2, g, z, out, counts, &bad) == RANK_NO_NEGATIVE);
        const int64_t h[2] = {1, 2147483648LL}, k[2] = {1, 2};
        EXPECT(rank_from_groups(2, h, k, out, counts, &bad) == RANK_NOT_CUMULATIVE && bad == 1);
        const int64_t neg[1] = {-1}, pos[1] = {3};
        EXPECT(rank_from_groups(1, neg, pos, out, counts, &bad) == RANK_NOT_CUMULATIVE && bad == 0);
    }
    std::printf("rank_host driver: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
