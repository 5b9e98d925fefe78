// Stand-alone driver of gem_amd/csrc/kmeans_host.hip (and of the matrix_host.hip scans k-means ingests with) for scripts/build_asan_kmeans.sh:
// every host function on small built cases, the results checked against values worked out by hand.  Plain C++, its own main; prints one summary line, exits non-zero on a wrong value.
#include "../../gem_amd/csrc/kmeans_host.hpp"
#include "../../gem_amd/csrc/matrix_host.hpp"
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
    // ---- checks
    {
        const int64_t n = 5; const int d = 3; const int64_t ld = 4;
        std::vector<float> X((size_t)n * ld, 1.f);
        for (int64_t i = 0; i < n; ++i) X[i * ld + 3] = std::numeric_limits<float>::quiet_NaN();          // padding: never read
        EXPECT(first_bad_entry(X.data(), n, d, ld, INFINITY) == -1);
        X[3 * ld + 2] = std::numeric_limits<float>::infinity();
        EXPECT(first_bad_entry(X.data(), n, d, ld, INFINITY) == 3 * d + 2);
        const int32_t lab[4] = {0, 2, 3, -1};
        EXPECT(first_bad_index(lab, 2, 3) == -1 && first_bad_index(lab, 4, 3) == 2 && first_bad_index(lab, 4, 4) == 3);
        const double u[4] = {0.0, 0.999, 1.0, std::numeric_limits<double>::quiet_NaN()};
        EXPECT(km_first_bad_uniform(u, 2) == -1 && km_first_bad_uniform(u, 4) == 2 && km_first_bad_uniform(u + 3, 1) == 0);
        const float V[6] = {1.f, 10.f, 3.f, 10.f, 5.f, 10.f};                                              // columns (1, 3, 5) and (10, 10, 10)
        EXPECT(std::fabs(km_mean_variance(V, 3, 2, 2) - (8.0 / 3.0) / 2.0) < 1e-15);
    }
    // ---- centre block, centres from sums, shift
    {
        const float C[6] = {1.f, 2.f, 3.f, -1.f, 0.f, 2.f};
        std::vector<float> Cp(32 * 8, -7.f), cn(32, -7.f);
        km_pad_centres(2, 3, 8, 32, C, Cp.data(), cn.data());
        EXPECT(Cp[0] == 1.f && Cp[2] == 3.f && Cp[3] == 0.f && Cp[8] == -1.f && Cp[10] == 2.f && Cp[16] == 0.f && Cp[32 * 8 - 1] == 0.f);
        EXPECT(cn[0] == 14.f && cn[1] == 5.f && std::isinf(cn[2]) && std::isinf(cn[31]));
        const double sums[16] = {3.0, 6.0, 9.0, 0, 0, 0, 0, 0, 1.0, 1.0, 1.0, 0, 0, 0, 0, 0};
        const int64_t counts[2] = {3, 0};
        float out[6];
        km_centres_from_sums(2, 3, 8, sums, counts, out);
        EXPECT(out[0] == 1.f && out[1] == 2.f && out[2] == 3.f && out[3] == 0.f && out[5] == 0.f);
        EXPECT(km_centre_shift(2, 3, C, out) == 1.0 + 0.0 + 4.0);
    }
    // ---- relocation
    {
        const double dist[7] = {1.0, 9.0, 0.5, 9.0, 2.0, 9.0, 0.0};
        int64_t far[3];
        km_relocation_order(7, dist, 3, far);
        EXPECT(far[0] == 1 && far[1] == 3 && far[2] == 5);
        km_relocation_order(7, dist, 1, far);
        EXPECT(far[0] == 1);
        int64_t all[7];
        km_relocation_order(7, dist, 9, all);                                                              // more asked for than there are rows
        EXPECT(all[3] == 4 && all[6] == 6);
        std::vector<double> sums = {-2.0, 0, 0.0, 0, 32.0, 0, 0.0, 0};                                     // K = 4, dpad = 2
        std::vector<int64_t> counts = {3, 0, 3, 0};
        const std::vector<int32_t> empty = {1, 3};
        const int32_t donor[2] = {0, 2};
        const float xrows[4] = {-3.f, 0.f, 13.f, 0.f};
        EXPECT(km_relocate(4, 2, empty, donor, xrows, sums.data(), counts.data()) == -1);
        EXPECT(sums[0] == 1.0 && sums[2] == -3.0 && sums[4] == 19.0 && sums[6] == 13.0);
        EXPECT(counts[0] == 2 && counts[1] == 1 && counts[2] == 2 && counts[3] == 1);
        std::vector<int64_t> lone = {2, 0, 1};
        std::vector<double> s2(6, 0.0);
        const std::vector<int32_t> e2 = {1};
        const int32_t d2[1] = {2};
        EXPECT(km_relocate(3, 2, e2, d2, xrows, s2.data(), lone.data()) == 0);                             // the donor would be emptied
        EXPECT(lone[1] == 0 && lone[2] == 1);
    }
    // ---- draws
    {
        EXPECT(km_first_row(0.0, 10) == 0 && km_first_row(0.999999, 10) == 9 && km_first_row(0.35, 10) == 3 && km_first_row(0.5, 1) == 0);
        const double prefix[5] = {0.0, 1.0, 1.0, 4.0, 4.5};
        EXPECT(km_find_block(prefix, 4, 0.0) == 0 && km_find_block(prefix, 4, 1.0) == 2 && km_find_block(prefix, 4, 4.2) == 3);
        EXPECT(km_find_block(prefix, 4, 4.5) == 4 && km_find_block(prefix, 0, 0.0) == 0);
        const float vals[4] = {0.f, 1.f, 0.f, 2.f};
        EXPECT(km_find_in_block(1.0, vals, 4, 1.0) == 1 && km_find_in_block(1.0, vals, 4, 2.0) == 3 && km_find_in_block(1.0, vals, 4, 4.0) == -1);
        EXPECT(km_find_in_block(0.0, vals, 0, 0.0) == -1);
    }
    // ---- scores
    {
        double out[4];
        const int64_t perfect[9] = {0, 5, 0, 7, 0, 0, 0, 0, 3};
        EXPECT(km_scores(perfect, 3, 3, out) && std::fabs(out[0] - 1.0) < 1e-12 && out[1] == 1.0 && out[2] == 1.0 && std::fabs(out[3] - 1.0) < 1e-12);
        const int64_t one[3] = {4, 4, 4};
        EXPECT(km_scores(one, 1, 3, out) && out[0] == 0.0 && out[1] == 0.0 && std::fabs(out[2] - 1.0 / 3.0) < 1e-15);
        const int64_t single[1] = {9};
        EXPECT(km_scores(single, 1, 1, out) && out[0] == 1.0 && out[1] == 1.0 && out[2] == 1.0);
        const int64_t big[4] = {1073741824, 3, 5, 1073741815};                                             // n = 2^31 - 1: n^2 and the pair products
        EXPECT(km_scores(big, 2, 2, out) && out[1] > 0.99 && out[1] < 1.0 && out[0] > 0.99);
        const int64_t neg[2] = {1, -1}, zero[2] = {0, 0};
        EXPECT(!km_scores(neg, 1, 2, out) && !km_scores(zero, 2, 1, out));
    }
    std::printf("kmeans_host driver: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
