// nbr_host.hip -- the device-free half of the neighbourhood link-prediction scores: see nbr_host.hpp.  Plain C++ in a .hip file so that the
// library's build picks it up.
#include "nbr_host.hpp"
#include <algorithm>
#include <cmath>

namespace gemhip {

int64_t nbr_first_bad_pair(int64_t n, int64_t m, const int32_t *st, const int32_t *ed, bool *self_pair)
{
    for (int64_t p = 0; p < m; ++p) {
        const bool outside = st[p] < 0 || st[p] >= n || ed[p] < 0 || ed[p] >= n;
        if (outside || st[p] == ed[p]) {
            *self_pair = !outside;
            return p;
        }
    }
    return -1;
}

void nbr_build_graph(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, std::vector<int64_t> &row_ptr, std::vector<int32_t> &col,
                     std::vector<int32_t> &deg)
{
    std::vector<int64_t> at((size_t)n + 1, 0);                // at[i + 1]: entries of row i before the dedupe, then the fill cursor of row i
    for (int64_t e = 0; e < m; ++e)
        if (src[e] != dst[e]) { ++at[(size_t)src[e] + 1]; ++at[(size_t)dst[e] + 1]; }
    for (int64_t i = 0; i < n; ++i) at[i + 1] += at[i];
    std::vector<int64_t> begin(at);                           // begin[i]: where row i starts before the dedupe
    col.assign((size_t)at[n], 0);
    for (int64_t e = 0; e < m; ++e)
        if (src[e] != dst[e]) { col[(size_t)at[src[e]]++] = dst[e]; col[(size_t)at[dst[e]]++] = src[e]; }
    row_ptr.assign((size_t)n + 1, 0);
    deg.assign((size_t)n, 0);
    int64_t w = 0;                                            // rows are compacted in place: the write cursor never passes a row's begin
    for (int64_t i = 0; i < n; ++i) {
        int32_t *lo = col.data() + begin[i], *hi = col.data() + begin[i + 1];
        std::sort(lo, hi);
        hi = std::unique(lo, hi);
        row_ptr[i] = w;
        deg[i] = (int32_t)(hi - lo);
        for (int32_t *q = lo; q < hi; ++q) col[(size_t)w++] = *q;
    }
    row_ptr[n] = w;
    col.resize((size_t)w);
}

void nbr_weights(int64_t n, const int32_t *deg, int which, double *w)
{
    for (int64_t i = 0; i < n; ++i) {
        const double d = (double)deg[i];
        if (which == 0) w[i] = deg[i] >= 2 ? 1.0 / std::log(d) : 0.0;
        else w[i] = deg[i] >= 1 ? 1.0 / d : 0.0;
    }
}

bool nbr_plan(const int32_t *deg, int64_t m, const int32_t *st, const int32_t *ed, NbrPlan &plan)
{
    plan = NbrPlan();
    for (int64_t p = 0; p < m; ++p) {
        const int32_t du = deg[st[p]], dv = deg[ed[p]];
        const int64_t la = nbr_first_is_a(du, dv, st[p], ed[p]) ? du : dv;
        if (la == 0) { ++plan.empty; continue; }
        plan.longest = std::max(plan.longest, std::min<int64_t>(la, NBR_CHUNK));
        if (la <= NBR_CHUNK) {
            (la <= NBR_NARROW ? plan.narrow : plan.wide).push_back(NbrItem{(int32_t)p, 0, (int32_t)la, -1});
            continue;
        }
        const int64_t pieces = (la + NBR_CHUNK - 1) / NBR_CHUNK;
        if (plan.slots + pieces > INT32_MAX) return false;
        plan.split.push_back(NbrSplit{(int32_t)p, (int32_t)plan.slots, (int32_t)pieces});
        for (int64_t k = 0; k < pieces; ++k) {
            const int64_t start = k * NBR_CHUNK, len = std::min<int64_t>(NBR_CHUNK, la - start);   // the last slice is partial
            (len <= NBR_NARROW ? plan.narrow : plan.wide).push_back(NbrItem{(int32_t)p, (int32_t)start, (int32_t)len, (int32_t)(plan.slots + k)});
        }
        plan.slots += pieces;
    }
    return true;
}

}  // namespace gemhip
