// sgns_plan.hpp -- the host arithmetic of SGNS (sgns_plan.hip): the Hogwild launch rule and the unigram alias tables.  Plain C++, no HIP:
// everything here runs on a CPU (scripts/build_asan_plan.sh, tests/test_sgns_plan.py), sgns_api.hip only uploads and launches what it returns.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

namespace gemhip {

// ---- what the rule shares with the kernels (sgns.hpp includes this header for them)
constexpr int SGNS_WAVE = 64;           // the wavefront width the kernels are written for (sgns.hpp asserts it equals gemhip::WAVE)
constexpr int SGNS_NEG = 5;             // SNAP: NegSamN = 5 (compile-time constant there too)
constexpr int HOGWILD_ROWS_PER_WAVE = 128;
// floats one cached row occupies in LDS and in the per-wave scratch row: RW = NV * VEC * 64 of the kernel the pickers INSTANTIATE for d
// (NV is 1, 2 or 4: three chunks run on the NV = 4 kernel, so d = 129..191 odd and 258..384 even occupy 256 / 512 floats, not 192 / 384;
// round 3 sized LDS and the scratch rows from the chunk count and the NV = 4 kernels wrote past both -- ADVICE r3)
inline int sgns_win_nv(int d) { const int nv = d % 2 == 0 ? (d + 127) / 128 : (d + 63) / 64; return nv <= 1 ? 1 : nv <= 2 ? 2 : 4; }
inline int sgns_win_row_floats(int d) { return sgns_win_nv(d) * (d % 2 == 0 ? 128 : 64); }

// How concentrated the row traffic of TrainModel is: what the Hogwild launch rule (plan_sgns_launch) needs to know about the vocabulary.
struct VocabStats {
    double n = 0.0, total = 0.0, max = 0.0, active = 0.0;     // table rows, tokens, largest count, nodes that occur at all
    double z = 0.0;                    // sum of count^0.75
    double n_eff = 0.0;                // 1 / sum_v q_v^2, q = unigram^0.75 distribution: the table size a uniform graph with the same collision rate would have
    double touch2 = 0.0;               // sum_v (p_v + 5 q_v)^2, p = token share: collision rate of the rows a (centre, context) pair TOUCHES (its context row + five negatives)
    mutable std::vector<int32_t> cnt_desc;     // token counts, descending (after sort_once), and ...
    mutable std::vector<double> u2_prefix;     // ... u2_prefix[i] = sum of (count^0.75)^2 over the i largest counts
    mutable std::vector<double> c_prefix, u_prefix;   // ... sums of count and of count^0.75 over the i largest counts
    void build(const int32_t *cnt, int64_t len)
    {
        double tot = 0.0, mx = 0.0, zz = 0.0, z2 = 0.0, c2 = 0.0, cu = 0.0;
        n = (double)len; active = 0.0;
        for (int64_t i = 0; i < len; ++i) {
            const int32_t c = cnt[i];
            if (c <= 0) continue;
            tot += c; mx = std::max(mx, (double)c); active += 1.0;
            const double u = std::pow((double)c, 0.75);
            zz += u; z2 += u * u; c2 += (double)c * c; cu += (double)c * u;
        }
        total = tot; max = mx; z = zz;
        n_eff = z2 > 0.0 ? zz * zz / z2 : n;
        touch2 = (tot > 0.0 && zz > 0.0) ? c2 / (tot * tot) + 10.0 * cu / (tot * zz) + 25.0 * z2 / (zz * zz) : 0.0;
        cnt_desc.assign(cnt, cnt + len);                     // sorted (and the prefix sums formed) only if the rule has to look at the cold rows
        u2_prefix.clear();
    }
    void sort_once() const
    {
        if (!u2_prefix.empty()) return;
        std::sort(cnt_desc.begin(), cnt_desc.end(), std::greater<int32_t>());
        u2_prefix.assign(cnt_desc.size() + 1, 0.0);
        c_prefix.assign(cnt_desc.size() + 1, 0.0); u_prefix.assign(cnt_desc.size() + 1, 0.0);
        for (size_t i = 0; i < cnt_desc.size(); ++i) {
            const double u = cnt_desc[i] > 0 ? std::pow((double)cnt_desc[i], 0.75) : 0.0;
            u2_prefix[i + 1] = u2_prefix[i] + u * u;
            c_prefix[i + 1] = c_prefix[i] + (cnt_desc[i] > 0 ? (double)cnt_desc[i] : 0.0);
            u_prefix[i + 1] = u_prefix[i] + u;
        }
    }
    // hot row-operations per trained (centre, context) pair when the rows with count >= thr are hot: P(the context is hot) + 5 x P(a negative is hot)
    double hot_ops_per_pair(double thr) const
    {
        if (cnt_desc.empty() || z <= 0.0 || total <= 0.0) return 0.0;
        sort_once();
        const size_t nhot = (size_t)(std::lower_bound(cnt_desc.begin(), cnt_desc.end(), thr, [](int32_t c, double t) { return (double)c >= t; }) - cnt_desc.begin());
        return c_prefix[nhot] / total + 5.0 * u_prefix[nhot] / z;
    }
    // effective table size of the negative-sampling distribution over the rows that are NOT hot (count < thr): hot rows take atomic adds and lose nothing
    double n_eff_cold(double thr) const
    {
        if (cnt_desc.empty() || z <= 0.0) return n;
        sort_once();
        const size_t nhot = (size_t)(std::lower_bound(cnt_desc.begin(), cnt_desc.end(), thr, [](int32_t c, double t) { return (double)c >= t; }) - cnt_desc.begin());
        const double s2 = (u2_prefix.back() - u2_prefix[nhot]) / (z * z);
        return s2 > 0.0 ? 1.0 / s2 : 1e300;
    }
};

// The knobs of a handle that steer the SGNS launch (gemhip_n2v_set_max_waves, gemhip_sgns_set_window_cache / _hogwild / _hot_rows) ...
struct SgnsKnobs {
    int32_t max_waves = 0;            // 0 = auto (plan_sgns_launch)
    int32_t cache_radius = -1;        // sgns_win_kernel LDS window radius: -1 auto, 0 = off (sgns_kernel)
    int32_t cache_delta = -1;         // -1 auto, 0 overwrite on leave, 1 delta write-back
    int32_t prefetch = 2;             // pairs whose negative rows are requested ahead: 2 (default) or 1 (d == 64/128/256.., whole window cached)
    int32_t reload = 1;               // Hogwild launches: update negative rows as they are at store time (second fetch) and the centre row by atomic add
    int32_t hot_count = -1;           // nodes with at least this many tokens never enter the LDS window: -1 auto (tokens / ((W-1) x (2R+1))), 0 off
    int32_t window_span = 0;          // positions of a walk whose context rows a wavefront holds at once: 0 = 2R+1 (the sliding window); the whole walk in the bucket kernel's whole-walk mode
    bool part = false;                // a bucket launch of the partitioned schedule (sgns_win_kernel<PART>: as-loaded window copies in global scratch, 3 wavefronts per SIMD)
    double duty = 1.0;                // fraction of a wavefront's time spent in pair steps (negative rows open); < 1 only for the buckets of the partitioned schedule
    double touch_scale = 1.0;         // factor on VocabStats::touch2 (bucket launches: the pairs of ONE bucket touch the rows of two partitions only: parts x duty)
    bool has_local_hot = false;       // this corpus HAS locally hot nodes (sgns_api.hip build_hotkey): the launch carries the staging row and a hot threshold even without count-hot rows
    int32_t local_hot = 8;            // LOCALLY HOT ROWS: a node with at least this many tokens per walk that contains it is treated as a hot row (0: off)
    int32_t neg_count = 0;            // fresh bit 2: token count from which a negative row is updated by atomic add (0: every row)
    int32_t fresh = 0;                // FRESH HOT ROWS (sgns.hpp, SgnsArgs::fresh): bit 0 hot centre words by returning atomics, bit 1 hot negatives re-read before the dot products
    bool node_id_layout = false;      // the unigram table the launch draws from is in node-id order (gemhip_n2v_build_unigram), not the binary's: half the concurrent-touch bound (plan_sgns_launch)
};
// The A/B overrides of a new handle's knobs: the GEMHIP_SGNS_* variables as `lookup` answers for them (gemhip_n2v_create passes getenv, once; the
// launch path reads no environment), each clamped to its knob's range; a variable `lookup` does not know leaves the default.
SgnsKnobs sgns_knobs_from_env(const char *(*lookup)(const char *));
// ... and what a launch of TrainModel over `nwalks` walks then looks like
struct SgnsLaunchPlan {
    bool window = false;              // sgns_win_kernel (LDS window) or sgns_kernel
    bool delta = false;               // window kernel: delta write-back (the Hogwild instantiation)
    int R = 0;                        // window radius
    int64_t waves = 1;                // concurrent wavefronts = concurrent walks
    int32_t hot_thr = 0;              // token count from which a row is "hot" (0: none)
    size_t lds = 0;                   // dynamic LDS bytes per workgroup
    int blocks = 1, threads = 64;
    // as the C ABI reports it: 0 sgns_kernel, 1 sgns_win_kernel (overwrite on leave), 2 sgns_win_kernel (Hogwild: delta write-back)
    int kernel() const { return !window ? 0 : delta ? 2 : 1; }
};

SgnsLaunchPlan plan_sgns_launch(const VocabStats &vs, const SgnsKnobs &kn, int64_t n, int32_t d, int32_t window, int32_t walk_len, int64_t nwalks, int32_t flags);

// The knobs and the vocabulary statistics of ONE bucket launch of the partitioned schedule (gemhip_sgns_train_part) on a handle whose knobs are `handle`
// and whose tables were built for `parts` partitions: vs_word = the statistics of the centre words' partition, vs_all = of the whole vocabulary;
// node_id_layout = the per-partition tables are in node-id order; corpus_hotkey = a hot key of the gathered corpus exists and names locally hot nodes
// (gemhip_n2v_locally_hot_corpus).  *vs_out: what plan_sgns_launch is to be called with.
SgnsKnobs bucket_knobs(const SgnsKnobs &handle, const VocabStats &vs_word, const VocabStats &vs_all, int32_t parts, int32_t walk_len, int32_t window,
                       int32_t flags, bool node_id_layout, bool corpus_hotkey, VocabStats *vs_out);

// InitUnigramTable (ELF @0x40e520) on a count vector: count^0.75, Vose in fp64, stacks popped from the back.  false: no entry has a positive count.
// U64 (optional): the table before the fp32 cast.
bool vose_unigram(const int32_t *cnt, int64_t n, int64_t stride, std::vector<float> &Uf, std::vector<int32_t> &K, std::vector<double> *U64 = nullptr);

// The unigram alias tables of all four gemhip_n2v_build_unigram* entry points.  Partition p = {v : v % parts == p}, local row v / parts, its rows at
// [part_off[p], part_off[p + 1]) of U / K / slot (one partition: local row = node id).
struct UnigramTables {
    std::vector<float> U;             // UTable by local row
    std::vector<int32_t> K;           // KTable by local row: the alias as a local row of the same partition
    std::vector<int32_t> slot;        // the binary's layout only: slot[part_off[p] + s] = the local row slot s of partition p names (flags & 2: its alias), -1 beyond part_slots[p]
    std::vector<int64_t> part_off;    // parts + 1 offsets
    std::vector<int64_t> part_slots;  // slots RndUnigramInt draws from per partition: its nodes that occur (the binary's layout) or all its rows (node-id layout)
    int64_t n_vocab = 0;              // their sum
    std::vector<VocabStats> vs_part;  // statistics of each partition's rows ...
    VocabStats vs;                    // ... and of the whole vocabulary
};
// counts[n]; order = nullptr: the node-id layout (every row of a partition is an entry of its table, in id order); order[n] = the nodes in order of
// first appearance in the corpus, those that never occur last: the binary's layout (a partition's table is over its nodes that occur, in that
// order -- LearnVocab's renaming, ELF @0x40d560).  Vose per partition over the counts in that order, stored by local row.  Returns -1, or the first
// partition whose vocabulary is empty (T is then incomplete; all-zero counts: 0, with T.n_vocab == 0 in the binary's layout).
int build_unigram_tables(const int32_t *counts, int64_t n, const int32_t *order, int32_t parts, int32_t flags, UnigramTables &T);

}  // namespace gemhip
