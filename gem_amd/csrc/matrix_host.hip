// matrix_host.hip -- the evaluation units' ingest checks (matrix_host.hpp).  No HIP header, no device code: builds with a plain C++ compiler.
#include "matrix_host.hpp"
#include <cmath>

namespace gemhip {

int64_t first_bad_entry(const float *X, int64_t n, int32_t d, int64_t ld, float max_abs)
{
    for (int64_t i = 0; i < n; ++i)
        for (int32_t c = 0; c < d; ++c) {
            const float v = X[i * ld + c];
            if (!std::isfinite(v) || std::fabs(v) > max_abs) return i * d + c;
        }
    return -1;
}

void pad_rows(const float *X, int64_t n, int32_t d, int64_t ld, int32_t dpad, float *out)
{
    for (int64_t i = 0; i < n; ++i)
        for (int32_t c = 0; c < dpad; ++c) out[i * dpad + c] = c < d ? X[i * ld + c] : 0.f;
}

int64_t first_bad_index(const int32_t *idx, int64_t m, int64_t n)
{
    for (int64_t t = 0; t < m; ++t)
        if (idx[t] < 0 || idx[t] >= n) return t;
    return -1;
}

int64_t first_bad_pair(const int32_t *st, const int32_t *ed, int64_t m, int64_t n)
{
    for (int64_t p = 0; p < m; ++p)
        if (st[p] < 0 || st[p] >= n || ed[p] < 0 || ed[p] >= n) return p;
    return -1;
}

}  // namespace gemhip
