// multi_plan.hip -- the schedules of the N-GPU entry points as host arithmetic (multi_plan.hpp).  No HIP include: compiles with `clang++ -x c++`.
#include "multi_plan.hpp"
#include <algorithm>
#include <cstring>

namespace gemhip {

Range shard_range(int64_t total, int64_t r, int64_t N) { return {total * r / N, total * (r + 1) / N}; }

GfRowBlocks gf_row_blocks(int64_t n, int N)
{
    const int64_t block = (n + N - 1) / N;
    return {n, block, block * N};
}

Range GfRowBlocks::rows(int r) const { return {std::min(r * block, n), std::min((r + 1) * block, n)}; }

GfShardError gf_check_shardable(int64_t n, int64_t m, const int32_t *src, const int32_t *dst)
{
    GfShardError err;
    int64_t last = -1;
    std::vector<char> seen((size_t)n, 0);
    for (int64_t e = 0; e < m; ++e) {
        if (src[e] < 0 || src[e] >= n || dst[e] < 0 || dst[e] >= n) { err.kind = GfShardError::EDGE_OUT_OF_RANGE; err.edge = e; return err; }
        if (dst[e] > src[e] && !seen[src[e]]) {
            seen[src[e]] = 1;
            if (src[e] < last) { err.kind = GfShardError::NOT_ASCENDING; err.edge = e; err.row = src[e]; err.after = last; return err; }
            last = src[e];
        }
    }
    return err;
}

N2vMultiPlan n2v_multi_plan(int64_t total_walks, int N, int episodes, int walk_len, int64_t n, int epochs)
{
    N2vMultiPlan P;
    P.N = N; P.episodes = episodes;
    P.prow = (n + N - 1) / N;
    for (int r = 0; r < N; ++r) {
        P.shard.push_back(shard_range(total_walks, r, N));
        P.shard_rows = std::max(P.shard_rows, P.shard[r].hi - P.shard[r].lo);
    }
    P.tab.resize((size_t)episodes * 3 * N);
    P.seg_len.assign(episodes, 1);
    for (int e = 0; e < episodes; ++e)
        for (int r = 0; r < N; ++r) {
            const Range s = shard_range(P.shard[r].hi - P.shard[r].lo, e, episodes);
            int64_t *t = P.tab.data() + (size_t)e * 3 * N;
            t[r] = r * P.shard_rows + s.lo; t[N + r] = s.hi - s.lo; t[2 * N + r] = P.shard[r].lo + s.lo;
            P.seg_len[e] = std::max(P.seg_len[e], s.hi - s.lo);
        }
    int64_t done = 0;
    for (int ep = 0; ep < epochs; ++ep)
        for (int e = 0; e < episodes; ++e) { P.token_offset.push_back(done); done += P.seg_len[e] * N * walk_len; }
    P.alpha_total = done;
    return P;
}

void partition_cut(const float *full, int64_t n, int d, int r, int N, float *part)
{
    const int64_t prow = (n + N - 1) / N;
    int64_t l = 0;
    for (; l * N + r < n; ++l) std::memcpy(part + (size_t)l * d, full + (size_t)(l * N + r) * d, (size_t)d * sizeof(float));
    std::fill(part + (size_t)l * d, part + (size_t)prow * d, 0.f);
}

void partition_paste(const float *part, int64_t n, int d, int r, int N, float *full)
{
    for (int64_t l = 0; l * N + r < n; ++l) std::memcpy(full + (size_t)(l * N + r) * d, part + (size_t)l * d, (size_t)d * sizeof(float));
}

}  // namespace gemhip
