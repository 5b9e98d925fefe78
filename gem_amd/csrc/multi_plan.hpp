// multi_plan.hpp -- the schedules of the N-GPU entry points (multi.hip) as host arithmetic: the balanced split, GF's row blocks and the edge orders that
// can be sharded by source row, node2vec's walk shards / episode table / alpha bookkeeping, and the cut and paste of a table partition.  Plain C++, no
// HIP: everything here runs on a CPU (scripts/build_asan_multi_plan.sh, tests/test_multi_plan.py, which holds it against gem_amd/multi_gpu.py);
// multi.hip only words the refusals and issues the device steps.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gemhip {

struct Range { int64_t lo, hi; };

// THE contiguous, balanced split of [0, total) over N parts (multi_gpu.py: shard_range): walks over ranks, a shard's walks over episodes
Range shard_range(int64_t total, int64_t r, int64_t N);

// GF: source rows in N contiguous blocks of `block` rows; the table is padded to n_pad = block * N rows so that every rank's block has one size
struct GfRowBlocks {
    int64_t n, block, n_pad;
    Range rows(int r) const;              // rank r's source rows, clamped to n (a rank past the end owns [n, n))
};
GfRowBlocks gf_row_blocks(int64_t n, int N);

// Can GF be sharded by source row?  Ranks read each other's rows from the PREVIOUS sweep's table: that is the reference's sweep only when no firing
// edge (dst > src) reads a row the reference has already updated in the same sweep, i.e. when the firing sources are first visited in ascending id
// order (gf.py:93-100 over graph.edges() of a graph whose nodes were inserted in id order -- every call site of the reference).
// multi_gpu.py: GFSharded.__init__ restates the rule on numpy arrays.
struct GfShardError {
    enum Kind { NONE = 0, EDGE_OUT_OF_RANGE, NOT_ASCENDING } kind = NONE;
    int64_t edge = -1;                    // the first offending edge (in list order, whichever kind comes first)
    int64_t row = -1, after = -1;         // NOT_ASCENDING: row `row` is first visited after the higher row `after`
    explicit operator bool() const { return kind != NONE; }
};
GfShardError gf_check_shardable(int64_t n, int64_t m, const int32_t *src, const int32_t *dst);

// node2vec on N ranks (multi_gpu.py: Node2VecPartitioned.episode_table / run).  Rank r walks shard[r] of the global walk ids; the gathered corpus
// gives every shard shard_rows rows (shorter shards padded); episode e trains the e-th slice of every shard.
struct N2vMultiPlan {
    int N = 0, episodes = 0;
    std::vector<Range> shard;             // [N] global walk ids
    int64_t shard_rows = 1;               // longest shard, at least 1
    std::vector<int64_t> tab;             // [episodes][3][N]: first corpus row, walks present, first global walk id of shard r's slice
    std::vector<int64_t> seg_len;         // [episodes] work items per shard = longest slice, at least 1 (an all-empty episode still moves alpha)
    std::vector<int64_t> token_offset;    // [epochs][episodes] tokens of the schedule in front of the episode
    int64_t alpha_total = 0;              // tokens of the whole schedule: epochs * sum_e seg_len[e] * N * walk_len
    int64_t prow = 0;                     // rows of a table partition: ceil(n / N)
    const int64_t *episode(int e) const { return tab.data() + (size_t)e * 3 * N; }
};
N2vMultiPlan n2v_multi_plan(int64_t total_walks, int N, int episodes, int walk_len, int64_t n, int epochs);

// Partition r of an n x d table: rows r, r + N, ... (node v -> partition v % N, local row v / N), zero-padded to ceil(n / N) rows; and its inverse
void partition_cut(const float *full, int64_t n, int d, int r, int N, float *part);
void partition_paste(const float *part, int64_t n, int d, int r, int N, float *full);

}  // namespace gemhip
