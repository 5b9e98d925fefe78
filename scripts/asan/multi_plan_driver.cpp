// Stand-alone driver of gem_amd/csrc/multi_plan.hip (the schedules of the N-GPU entry points: balanced split, GF row blocks and the shardable-order
// rule, node2vec's shards / episode table / alpha bookkeeping, cut and paste of a table partition): plain C++, no HIP, no device.
//
//   multi_plan_driver shard <total> <N>                stdout: "lo hi" of shard_range(total, r, N), one line per r
//   multi_plan_driver blocks <n> <N>                   stdout: "block n_pad", then "r0 r1" of GfRowBlocks::rows(r), one line per r
//   multi_plan_driver n2v <total> <N> <episodes> <walk_len> <n> <epochs> <out>
//       out: int64 shard_rows, prow, alpha_total; shard[N][2]; tab[episodes][3][N]; seg_len[episodes]; token_offset[epochs][episodes]
//   multi_plan_driver gfcheck <in> <out>
//       in:  int64 count; then per edge list: int64 n, m; int32 src[m]; int32 dst[m]        out: per list int64 kind, edge, row, after
//   multi_plan_driver parts <in> <out>
//       in:  int64 n, d, N; float full[n * d]
//       out: partition_cut of r = 0 .. N-1 (ceil(n / N) * d floats each, the buffers pre-filled with NaN), then partition_paste of all of them into an
//            n * d buffer pre-filled with NaN
//   multi_plan_driver self
//       the corners of tests/test_multi_plan.py with built-in expectations; exit status 1 when one fails
//
// tests/test_multi_plan.py uses the file forms; scripts/build_asan_multi_plan.sh runs `self` under AddressSanitizer and UBSan.
#include "../../gem_amd/csrc/multi_plan.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

using namespace gemhip;

namespace {

template <typename T> bool read_vec(FILE *f, std::vector<T> &v, int64_t count)
{
    v.resize((size_t)count);
    return count == 0 || fread(v.data(), sizeof(T), (size_t)count, f) == (size_t)count;
}
template <typename T> void write_vec(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int run_n2v(char **a)
{
    const int N = atoi(a[1]), episodes = atoi(a[2]);
    const N2vMultiPlan P = n2v_multi_plan(atoll(a[0]), N, episodes, atoi(a[3]), atoll(a[4]), atoi(a[5]));
    FILE *o = fopen(a[6], "wb");
    if (!o) { fprintf(stderr, "multi_plan_driver: cannot write %s\n", a[6]); return 2; }
    std::vector<int64_t> head{P.shard_rows, P.prow, P.alpha_total};
    for (const Range &s : P.shard) { head.push_back(s.lo); head.push_back(s.hi); }
    write_vec(o, head); write_vec(o, P.tab); write_vec(o, P.seg_len); write_vec(o, P.token_offset);
    return fclose(o) ? 2 : 0;
}

int run_gfcheck(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb"), *o = fopen(out_path, "wb");
    int64_t count = 0;
    if (!f || !o || fread(&count, 8, 1, f) != 1) { fprintf(stderr, "multi_plan_driver: bad input %s\n", in_path); return 2; }
    for (int64_t k = 0; k < count; ++k) {
        int64_t hdr[2];
        std::vector<int32_t> src, dst;
        if (fread(hdr, 8, 2, f) != 2 || !read_vec(f, src, hdr[1]) || !read_vec(f, dst, hdr[1])) { fprintf(stderr, "multi_plan_driver: bad input %s\n", in_path); return 2; }
        const GfShardError e = gf_check_shardable(hdr[0], hdr[1], src.data(), dst.data());
        const int64_t out[4] = {(int64_t)e.kind, e.edge, e.row, e.after};
        fwrite(out, 8, 4, o);
    }
    fclose(f);
    return fclose(o) ? 2 : 0;
}

int run_parts(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb");
    int64_t hdr[3];
    std::vector<float> full;
    if (!f || fread(hdr, 8, 3, f) != 3 || !read_vec(f, full, hdr[0] * hdr[1])) { fprintf(stderr, "multi_plan_driver: bad input %s\n", in_path); return 2; }
    fclose(f);
    const int64_t n = hdr[0]; const int d = (int)hdr[1], N = (int)hdr[2];
    const int64_t prow = (n + N - 1) / N;
    FILE *o = fopen(out_path, "wb");
    if (!o) { fprintf(stderr, "multi_plan_driver: cannot write %s\n", out_path); return 2; }
    std::vector<float> back((size_t)n * d, NAN);
    for (int r = 0; r < N; ++r) {
        std::vector<float> part((size_t)prow * d, NAN);
        partition_cut(full.data(), n, d, r, N, part.data());
        partition_paste(part.data(), n, d, r, N, back.data());
        write_vec(o, part);
    }
    write_vec(o, back);
    return fclose(o) ? 2 : 0;
}

// ---- self checks
int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

void check_shards(int64_t total, int N)
{
    int64_t at = 0;
    for (int r = 0; r < N; ++r) {
        const Range s = shard_range(total, r, N);
        EXPECT(s.lo == at && s.hi >= s.lo && s.hi - s.lo <= total / N + 1 && s.hi - s.lo >= total / N, "shard_range(%lld, %d, %d) = [%lld, %lld)", (long long)total, r, N, (long long)s.lo, (long long)s.hi);
        at = s.hi;
    }
    EXPECT(at == total, "shard_range(%lld, ., %d) ends at %lld", (long long)total, N, (long long)at);
}

void check_blocks(int64_t n, int N)
{
    const GfRowBlocks B = gf_row_blocks(n, N);
    EXPECT(B.n_pad % N == 0 && B.n_pad >= n && B.n_pad - n < N && B.block * N == B.n_pad, "blocks(%lld, %d): block %lld n_pad %lld", (long long)n, N, (long long)B.block, (long long)B.n_pad);
    int64_t at = 0;
    for (int r = 0; r < N; ++r) {
        const Range b = B.rows(r);
        EXPECT(b.lo == at && b.hi >= b.lo && b.hi <= n && b.lo == std::min<int64_t>(r * B.block, n), "blocks(%lld, %d): rank %d owns [%lld, %lld)", (long long)n, N, r, (long long)b.lo, (long long)b.hi);
        at = b.hi;
    }
    EXPECT(at == n, "blocks(%lld, %d) end at %lld", (long long)n, N, (long long)at);
}

// every walk of [0, total) in exactly one slice, slices of a shard in corpus-row order; seg_len, offsets and alpha_total as the sums say
void check_n2v(int64_t total, int N, int episodes, int walk_len, int64_t n, int epochs)
{
    const N2vMultiPlan P = n2v_multi_plan(total, N, episodes, walk_len, n, epochs);
    std::vector<int> seen((size_t)total, 0);
    int64_t rows = 1, tokens = 0;
    for (int r = 0; r < N; ++r) rows = std::max(rows, P.shard[r].hi - P.shard[r].lo);
    EXPECT(P.shard_rows == rows && P.prow == (n + N - 1) / N, "n2v(%lld, %d): shard_rows %lld prow %lld", (long long)total, N, (long long)P.shard_rows, (long long)P.prow);
    for (int e = 0; e < episodes; ++e) {
        const int64_t *t = P.episode(e);
        int64_t longest = 1;
        for (int r = 0; r < N; ++r) {
            for (int64_t j = 0; j < t[N + r]; ++j) {
                const int64_t id = t[2 * N + r] + j;
                EXPECT(id >= P.shard[r].lo && id < P.shard[r].hi && t[r] + j == r * P.shard_rows + (id - P.shard[r].lo), "n2v(%lld, %d, %d): episode %d shard %d walk %lld", (long long)total, N, episodes, e, r, (long long)id);
                if (id >= 0 && id < total) ++seen[(size_t)id];
            }
            longest = std::max(longest, t[N + r]);
        }
        EXPECT(P.seg_len[e] == longest, "n2v(%lld, %d, %d): seg_len[%d] = %lld", (long long)total, N, episodes, e, (long long)P.seg_len[e]);
        tokens += longest * N * walk_len;
    }
    EXPECT(std::all_of(seen.begin(), seen.end(), [](int c) { return c == 1; }), "n2v(%lld, %d, %d): a walk is in no slice or in two", (long long)total, N, episodes);
    EXPECT(P.alpha_total == tokens * epochs && (int)P.token_offset.size() == epochs * episodes, "n2v(%lld, %d, %d): alpha_total %lld", (long long)total, N, episodes, (long long)P.alpha_total);
    int64_t done = 0;
    for (int k = 0; k < epochs * episodes; ++k) { EXPECT(P.token_offset[k] == done, "n2v(%lld, %d, %d): offset %d", (long long)total, N, episodes, k); done += P.seg_len[k % episodes] * N * walk_len; }
}

void check_parts(int64_t n, int N, int d)
{
    std::vector<float> full((size_t)n * d), back((size_t)n * d, NAN);
    for (size_t i = 0; i < full.size(); ++i) full[i] = 1.f + (float)i;
    const int64_t prow = (n + N - 1) / N;
    for (int r = 0; r < N; ++r) {
        std::vector<float> part((size_t)prow * d, NAN);
        partition_cut(full.data(), n, d, r, N, part.data());
        for (int64_t l = 0; l < prow; ++l)
            for (int k = 0; k < d; ++k) {
                const float want = l * N + r < n ? full[(size_t)(l * N + r) * d + k] : 0.f;
                EXPECT(part[(size_t)l * d + k] == want, "parts(%lld, %d, %d): partition %d row %lld", (long long)n, N, d, r, (long long)l);
            }
        partition_paste(part.data(), n, d, r, N, back.data());
    }
    EXPECT(!memcmp(full.data(), back.data(), full.size() * sizeof(float)), "parts(%lld, %d, %d): paste of all cuts", (long long)n, N, d);
}

void check_gf(const char *what, int64_t n, const std::vector<int32_t> &src, const std::vector<int32_t> &dst, GfShardError::Kind kind, int64_t edge, int64_t row, int64_t after)
{
    const GfShardError e = gf_check_shardable(n, (int64_t)src.size(), src.data(), dst.data());
    EXPECT(e.kind == kind && e.edge == edge && e.row == row && e.after == after, "%s: kind %d edge %lld row %lld after %lld", what, (int)e.kind, (long long)e.edge, (long long)e.row, (long long)e.after);
    EXPECT((bool)e == (kind != GfShardError::NONE), "%s: operator bool", what);
}

int run_self()
{
    for (int64_t total : {0, 1, 2, 5, 6, 1000, 1024})
        for (int N : {1, 2, 3, 4, 7, 8, 64}) {
            check_shards(total, N);
            for (int episodes : {1, 3, 64}) check_n2v(total, N, episodes, 8, 1001, 2);
        }
    check_n2v(24, 4, 3, 5, 6, 1);                          // divisible by N * episodes: every slice has 2 walks
    {
        const N2vMultiPlan P = n2v_multi_plan(6, 4, 3, 8, 6, 1);      // shards of 1, 2, 1, 2 walks: slices 0 0 1 / 0 1 1 per shard, seg_len at least 1
        const int64_t want[] = {0, 2, 4, 6,  0, 0, 0, 0,  0, 1, 3, 4,   0, 2, 4, 6,  0, 1, 0, 1,  0, 1, 3, 4,   0, 3, 4, 7,  1, 1, 1, 1,  0, 2, 3, 5};
        EXPECT(P.tab.size() == 36 && !memcmp(P.tab.data(), want, sizeof want), "n2v(6, 4, 3): episode table");
        EXPECT(P.shard_rows == 2 && P.prow == 2 && (P.seg_len == std::vector<int64_t>{1, 1, 1}) && P.alpha_total == 96 && (P.token_offset == std::vector<int64_t>{0, 32, 64}), "n2v(6, 4, 3): scalars");
    }
    const int blocks[][2] = {{4, 4}, {5, 4}, {3, 4}, {1001, 4}, {1001, 1}};
    for (const auto &c : blocks) check_blocks(c[0], c[1]);
    { const GfRowBlocks B = gf_row_blocks(5, 4); EXPECT(B.block == 2 && B.n_pad == 8 && B.rows(2).lo == 4 && B.rows(2).hi == 5 && B.rows(3).lo == 5 && B.rows(3).hi == 5, "blocks(5, 4): the last rank owns [5, 5)"); }
    { const GfRowBlocks B = gf_row_blocks(4, 4); EXPECT(B.block == 1 && B.n_pad == 4, "blocks(4, 4): no padding"); }
    for (int64_t n : {1, 5, 8, 1001})
        for (int N : {1, 3, 4, 8})
            for (int d : {1, 16}) check_parts(n, N, d);

    using E = GfShardError;
    check_gf("ascending path", 4, {0, 1, 2}, {1, 2, 3}, E::NONE, -1, -1, -1);
    check_gf("no edges", 3, {}, {}, E::NONE, -1, -1, -1);
    check_gf("a revisited row is no new visit", 4, {0, 2, 0, 3}, {1, 3, 2, 1}, E::NONE, -1, -1, -1);
    check_gf("edges that do not fire never count", 4, {3, 2, 0, 1}, {0, 1, 1, 2}, E::NONE, -1, -1, -1);
    check_gf("row 1 after row 2", 4, {0, 2, 1}, {1, 3, 2}, E::NOT_ASCENDING, 2, 1, 2);
    check_gf("row 0 after row 3, behind a non-firing edge", 5, {3, 4, 0}, {4, 0, 1}, E::NOT_ASCENDING, 2, 0, 3);
    check_gf("dst = n", 3, {0, 1}, {1, 3}, E::EDGE_OUT_OF_RANGE, 1, -1, -1);
    check_gf("src < 0", 3, {-1, 1}, {1, 2}, E::EDGE_OUT_OF_RANGE, 0, -1, -1);
    check_gf("the order fails before the bad edge", 4, {2, 1, 9}, {3, 2, 0}, E::NOT_ASCENDING, 1, 1, 2);
    // random lists against the rule restated on the order of first visits
    std::mt19937 mt(11);
    int accepted = 0, refused = 0;
    for (int k = 0; k < 200; ++k) {
        const int n = 1 + (int)(mt() % 12), m = (int)(mt() % 31);
        std::vector<int32_t> src(m), dst(m);
        for (int e = 0; e < m; ++e) { src[e] = (int32_t)(mt() % (uint32_t)n); dst[e] = (int32_t)(mt() % (uint32_t)n); }
        if (k & 1) {                                      // grouped by ascending source: always shardable
            std::vector<int> idx(m);
            for (int e = 0; e < m; ++e) idx[e] = e;
            std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return src[a] < src[b]; });
            std::vector<int32_t> s2(m), d2(m);
            for (int e = 0; e < m; ++e) { s2[e] = src[idx[e]]; d2[e] = dst[idx[e]]; }
            src = s2; dst = d2;
        }
        std::vector<int32_t> visits; std::vector<int> at;
        for (int e = 0; e < m; ++e) if (dst[e] > src[e] && std::find(visits.begin(), visits.end(), src[e]) == visits.end()) { visits.push_back(src[e]); at.push_back(e); }
        size_t bad = 1;
        while (bad < visits.size() && visits[bad] > visits[bad - 1]) ++bad;
        if (bad < visits.size()) { check_gf("random list", n, src, dst, E::NOT_ASCENDING, at[bad], visits[bad], visits[bad - 1]); ++refused; }
        else { check_gf("random list", n, src, dst, E::NONE, -1, -1, -1); ++accepted; }
    }
    EXPECT(accepted >= 40 && refused >= 40, "random lists: %d accepted, %d refused", accepted, refused);
    fprintf(stderr, "multi plan driver: %d failed checks\n", failures);
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "shard")) {
        for (int r = 0; r < atoi(argv[3]); ++r) { const Range s = shard_range(atoll(argv[2]), r, atoi(argv[3])); printf("%lld %lld\n", (long long)s.lo, (long long)s.hi); }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "blocks")) {
        const GfRowBlocks B = gf_row_blocks(atoll(argv[2]), atoi(argv[3]));
        printf("%lld %lld\n", (long long)B.block, (long long)B.n_pad);
        for (int r = 0; r < atoi(argv[3]); ++r) printf("%lld %lld\n", (long long)B.rows(r).lo, (long long)B.rows(r).hi);
        return 0;
    }
    if (argc == 9 && !strcmp(argv[1], "n2v")) return run_n2v(argv + 2);
    if (argc == 4 && !strcmp(argv[1], "gfcheck")) return run_gfcheck(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "parts")) return run_parts(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "self")) return run_self();
    fprintf(stderr, "usage: %s shard <total> <N> | blocks <n> <N> | n2v <total> <N> <episodes> <walk_len> <n> <epochs> <out> | gfcheck <in> <out> | parts <in> <out> | self\n", argv[0]);
    return 2;
}
