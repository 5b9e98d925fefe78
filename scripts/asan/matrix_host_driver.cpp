// Stand-alone driver of gem_amd/csrc/matrix_host.hip (tests/test_matrix_host.py; also fit for a sanitizer build): every function on small
// built cases, the results checked against values worked out by hand.  Every buffer has exactly the size the function may touch, so a read
// of a padding column past the last row, or a write past dpad, is out of bounds.  Plain C++, its own main; prints one summary line, exits
// non-zero on a wrong value.
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
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- first_bad_entry
    {
        const float one[3] = {1.f, -2.f, 3.f};                                                             // n = 1, d = ld
        EXPECT(first_bad_entry(one, 1, 3, 3, INFINITY) == -1);
        const float one_bad[3] = {1.f, -2.f, nan};
        EXPECT(first_bad_entry(one_bad, 1, 3, 3, INFINITY) == 2 && first_bad_entry(one_bad, 1, 2, 3, INFINITY) == -1);
        const int64_t n = 5; const int d = 3; const int64_t ld = 4;
        std::vector<float> X((size_t)n * ld, 1.f);
        for (int64_t i = 0; i < n; ++i) X[i * ld + 3] = nan;                                               // padding: never read
        EXPECT(first_bad_entry(X.data(), n, d, ld, INFINITY) == -1);
        EXPECT(first_bad_entry(X.data(), n, 4, ld, INFINITY) == 3);                                        // d = ld: the same column counts
        X[3 * ld + 2] = inf;
        EXPECT(first_bad_entry(X.data(), n, d, ld, INFINITY) == 3 * d + 2);
        X[4 * ld + 0] = nan;                                                                               // a later offender: the first is named
        EXPECT(first_bad_entry(X.data(), n, d, ld, INFINITY) == 3 * d + 2);
        X[1 * ld + 1] = -inf;
        EXPECT(first_bad_entry(X.data(), n, d, ld, INFINITY) == 1 * d + 1);
        std::vector<float> last((size_t)n * d, 0.5f);                                                      // the last entry of the last row
        last[(size_t)n * d - 1] = -inf;
        EXPECT(first_bad_entry(last.data(), n, d, d, INFINITY) == n * d - 1);
    }
    // ---- the magnitude bound is inclusive
    {
        const float bound = 1e18f, above = std::nextafter(bound, inf);
        float X[6] = {0.f, bound, -bound, 1.f, 2.f, 3.f};
        EXPECT(first_bad_entry(X, 2, 3, 3, bound) == -1);
        X[5] = -above;
        EXPECT(first_bad_entry(X, 2, 3, 3, bound) == 5 && first_bad_entry(X, 2, 3, 3, INFINITY) == -1);
        X[4] = nan;                                                                                        // not finite comes first in position
        EXPECT(first_bad_entry(X, 2, 3, 3, bound) == 4);
        X[2] = above;
        EXPECT(first_bad_entry(X, 2, 3, 3, bound) == 2);
        const float big[2] = {std::numeric_limits<float>::max(), -std::numeric_limits<float>::max()};
        EXPECT(first_bad_entry(big, 1, 2, 2, INFINITY) == -1 && first_bad_entry(big, 1, 2, 2, 0.f) == 0);
    }
    // ---- pad_rows
    {
        const float X[8] = {1.f, 2.f, 3.f, nan, 4.f, 5.f, 6.f, nan};                                       // [2][4], d = 3
        std::vector<float> same(6, -7.f), wide(16, -7.f);
        pad_rows(X, 2, 3, 4, 3, same.data());                                                              // dpad = d
        EXPECT(same[0] == 1.f && same[2] == 3.f && same[3] == 4.f && same[5] == 6.f);
        pad_rows(X, 2, 3, 4, 8, wide.data());                                                              // dpad > d
        EXPECT(wide[0] == 1.f && wide[2] == 3.f && wide[8] == 4.f && wide[10] == 6.f);
        for (int c = 3; c < 8; ++c) EXPECT(wide[c] == 0.f && wide[8 + c] == 0.f);
        float one_out[2] = {-7.f, -7.f};
        pad_rows(X, 1, 1, 4, 2, one_out);                                                                  // n = 1
        EXPECT(one_out[0] == 1.f && one_out[1] == 0.f);
        pad_rows(X, 0, 3, 4, 8, nullptr);                                                                  // no rows: nothing is touched
    }
    // ---- index and pair lists
    {
        const int32_t lab[4] = {0, 2, 3, -1};
        EXPECT(first_bad_index(lab, 2, 3) == -1 && first_bad_index(lab, 4, 3) == 2 && first_bad_index(lab, 4, 4) == 3);
        EXPECT(first_bad_index(lab, 0, 3) == -1 && first_bad_index(nullptr, 0, 3) == -1);                  // empty lists
        const int32_t low[2] = {1, std::numeric_limits<int32_t>::min()};
        EXPECT(first_bad_index(low, 2, 2) == 1 && first_bad_index(low, 1, 2) == -1);
        const int32_t top[1] = {std::numeric_limits<int32_t>::max()};
        EXPECT(first_bad_index(top, 1, (int64_t)1 << 31) == -1 && first_bad_index(top, 1, std::numeric_limits<int32_t>::max()) == 0);
        const int32_t st[4] = {0, 1, 2, 2}, ed[4] = {1, 1, 5, -1};
        EXPECT(first_bad_pair(st, ed, 2, 3) == -1);                                                        // st == ed is no fault here
        EXPECT(first_bad_pair(st, ed, 4, 3) == 2 && first_bad_pair(st, ed, 4, 6) == 3 && first_bad_pair(ed, st, 4, 6) == 3);
        EXPECT(first_bad_pair(st, ed, 0, 3) == -1 && first_bad_pair(nullptr, nullptr, 0, 3) == -1);
        EXPECT(first_bad_pair(st, low, 2, 3) == 1 && first_bad_pair(low, st, 2, 3) == 1);
    }
    std::printf("matrix_host driver: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
