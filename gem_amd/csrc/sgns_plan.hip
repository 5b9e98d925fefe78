// sgns_plan.hip -- the host arithmetic of SGNS on gfx950: the Hogwild launch rule (which kernel, how many wavefronts, which rows are hot), the knobs of
// a bucket launch of the partitioned schedule, and the unigram alias tables of InitUnigramTable in both layouts, for one table or one per partition.
// HIP-free by rule: no HIP header, nothing from common.hpp -- the `.hip` suffix only serves the build's csrc/*.hip glob, and the file is also valid
// `clang++ -x c++ -std=c++17` input (scripts/build_asan_plan.sh runs it under AddressSanitizer / UBSan with a driver of its own, tests/test_sgns_plan.py
// compares that driver's output with tests/golden/sgns_plan_grid.txt and the tables with the oracle's).  sgns_api.hip holds the C ABI around it.
#include "sgns_plan.hpp"
#include "../../include/gem_hip.h"
#include <cstdlib>

namespace gemhip {

SgnsKnobs sgns_knobs_from_env(const char *(*lookup)(const char *))
{
    SgnsKnobs kn;
    if (const char *e = lookup("GEMHIP_SGNS_MAX_WAVES")) kn.max_waves = std::max(0, atoi(e));
    if (const char *e = lookup("GEMHIP_SGNS_CACHE_R")) kn.cache_radius = std::min(31, std::max(-1, atoi(e)));
    if (const char *e = lookup("GEMHIP_SGNS_CACHE_DELTA")) kn.cache_delta = std::min(1, std::max(-1, atoi(e)));
    if (const char *e = lookup("GEMHIP_SGNS_PREFETCH")) kn.prefetch = std::min(2, std::max(1, atoi(e)));
    if (const char *e = lookup("GEMHIP_SGNS_RELOAD")) kn.reload = atoi(e) != 0;
    if (const char *e = lookup("GEMHIP_SGNS_HOT_COUNT")) kn.hot_count = std::max(-1, atoi(e));
    if (const char *e = lookup("GEMHIP_SGNS_LOCAL_HOT")) kn.local_hot = std::max(0, atoi(e));
    if (const char *e = lookup("GEMHIP_SGNS_FRESH")) kn.fresh = atoi(e) & 7;
    if (const char *e = lookup("GEMHIP_SGNS_NEG_COUNT")) kn.neg_count = std::max(0, atoi(e));
    return kn;
}

// Which kernel, how many concurrent wavefronts and which rows are "hot" for one pass of TrainModel over `nwalks` walks.  Pure host arithmetic.
//
// Concurrency against quality -- the rule and where it comes from.  What Hogwild costs here is LOST UPDATES: every wavefront
// keeps its 5 negative rows per pair open from their load to their store; a store another wavefront makes to such a row in between is
// overwritten.  The CPU replay of this kernel's concurrency (scripts/hogwild_emul: W virtual wavefronts, the kernel's private copies) puts
// ~90 % of the MAP loss on those overwritten negative-row updates, ~10 % on the centre row's, none on stale gradients; the expected fraction
// of overwriting stores is  rho = W x 5 x w / n_eff  with w = the window in pair steps (prefetch + 1 without RELOAD; ~0.4 with it: one reload
// round trip, ~0.5 us against a 1.35 us step) and n_eff = 1 / sum_v q_v^2 the EFFECTIVE table size of the negative-sampling distribution
// (unigram^0.75): n on a graph whose nodes are equally frequent (SBM: n / 1.06), far smaller on a power-law graph (R-MAT scale 17: 11 316 of
// 131 072 nodes).  Measured at SBM 1M/10M against the sequential oracle (same seed, paired per-node AP): without RELOAD rho = 1.1 % / 1.5 % /
// 2.3 % (768 / 1024 / 1536 wavefronts) cost -0.1 % / -0.4..-0.9 % / -0.8..-1.3 % of MAP, and 1536 wavefronts with prefetch 1 (rho 1.5 %)
// -0.5 %: the loss follows rho, not the wavefront count; with RELOAD 1536 wavefronts (rho 0.3 %) measure +0.15 +- 0.25 %.  Default: rho <= 1.5 %.
SgnsLaunchPlan plan_sgns_launch(const VocabStats &vs, const SgnsKnobs &kn, int64_t n, int32_t d, int32_t window, int32_t walk_len,
                                       int64_t nwalks, int32_t flags)
{
    SgnsLaunchPlan P;
    const bool deterministic = (flags & 4) != 0;
    // window-cached kernel (default): radius R = tokens either side of the centre whose SynPos row stays in LDS
    int R = kn.cache_radius < 0 ? 10 : kn.cache_radius;
    R = std::min(R, std::min(window, 31));
    const int rw = sgns_win_row_floats(d);
    const size_t ints = (size_t)((walk_len + 4 * window * SGNS_NEG + 3) & ~3);
    // tokens + negative targets of two centres, the window rows (twice with the delta write-back: as trained / as loaded) and -- unless every context
    // row is cached (`allc`: R >= window and no hot rows, the launcher's ALLC instantiations) -- one staging row for an uncached context
    // (kn.part: the bucket kernels keep the as-loaded copies in a global scratch instead of LDS)
    auto lds_bytes = [&](bool delta, bool allc) { return ints * sizeof(int32_t) + (size_t)((2 * R + 1) * ((delta && !kn.part) ? 2 : 1) + (allc ? 0 : 1)) * rw * sizeof(float); };
    // the window has to fit a block's LDS: wide rows / long walks fall back to sgns_kernel
    P.window = R > 0 && !(flags & GEMHIP_N2V_NO_WINDOW_CACHE) && 2 * window * SGNS_NEG <= 2 * SGNS_WAVE && walk_len >= 2 && lds_bytes(true, false) <= 64 * 1024 &&
               (d % 2 == 0 ? d <= 512 : d <= 256);
    if (!P.window) {
        // sgns_kernel: four wavefronts per workgroup, no private copies beyond the pair in flight.  Small graphs: when the open rows approach n,
        // concurrent writers overwrite each other's updates and the embedding degrades (tests/test_n2v_gpu.py): n / 128 wavefronts
        const size_t per_wave = (size_t)(walk_len + 2 * window * SGNS_NEG) * sizeof(int32_t);
        if (!deterministic) {
            const int64_t hog_cap = kn.max_waves > 0 ? kn.max_waves : std::max<int64_t>(1, n / HOGWILD_ROWS_PER_WAVE);
            P.waves = std::min<int64_t>(std::min<int64_t>(hog_cap, 256 * 16), nwalks);          // 16 waves/CU already saturate the fabric (scripts/ab_sgns_waves.py)
            P.threads = 256; P.blocks = (int)((P.waves + 3) / 4);
        }
        P.lds = per_wave * (P.threads / 64);
        return P;
    }
    P.R = R;
    const int mode = kn.cache_delta;                 // -1 auto: delta write-back whenever other wavefronts train concurrently
    P.delta = deterministic && mode == 1;            // (cache_delta 1 on a deterministic launch: the Hogwild code path on ONE wavefront, for the parity tests)
    // a node expected to sit in another wavefront's window at any time -- (W - 1) x (2R + 1) x count / tokens >= 1 -- is hot
    const double span = kn.window_span > 0 ? (double)kn.window_span : (double)(2 * R + 1);
    auto hot_threshold = [&](int64_t waves) -> int32_t {
        if (kn.hot_count > 0) return kn.hot_count;
        if (kn.hot_count < 0 && waves > 1 && vs.total > 0.0) {
            const double thr = vs.total / ((double)(waves - 1) * span);
            if (vs.max >= thr) return (int32_t)std::max(2.0, std::ceil(thr));
        }
        return 0;
    };
    bool allc = R >= window && !kn.has_local_hot;
    if (!deterministic) {
        P.delta = mode != 0;
        // the (reload, prefetch) pair the launcher will actually run: launches WITHOUT reload-on-update and with prefetch distance 1 exist for the
        // benchmark shape only (d == 128, whole window cached, no hot rows -- launch_sgns_win's AB instantiations); every other Hogwild launch is
        // reload-on-update with prefetch distance 2 whatever the knobs say, and the width rule has to be computed for THAT kernel
        auto w_steps_of = [&](bool all_cached) -> double {
            const bool ab_shape = d == 128 && all_cached;
            const bool reload_eff = P.delta && (kn.reload || !ab_shape);
            return reload_eff ? 0.4 : (double)((ab_shape ? kn.prefetch : 2) + 1);
        };
        const double n_eff = vs.n_eff > 0.0 ? vs.n_eff : (double)n;
        // graphs below 8192 nodes: the window rows themselves (2R+1 per wavefront) are a sizeable part of the table -- SBM-1024 (d=16) loses
        // 3.5 % of MAP at 8 wavefronts and nothing at 2: bound the open fraction of the table at 1/16
        const int64_t hog_tiny = std::max<int64_t>(1, n / (16 * (8 + 2 * R + 1)));
        // ... but never more wavefronts than 2 % of the rows that occur at all: that is as far as the measurements behind this rule reach (stale
        // gradients cost nothing up to there -- CPU replay at 0.4 %, SBM 100k at 0.8 %, R-MAT scale 17 at 2.0 % of the active rows; R-MAT scale 13 with
        // 26 % of its 5 936 active rows open ended 21 % ABOVE the sequential algorithm's MAP: its hubs under-trained)
        const int64_t w_act = std::max<int64_t>(1, (int64_t)((vs.active > 0.0 ? vs.active : (double)n) / 50.0));
        // ... and, on graphs with hubs, never more than the CONCURRENT-TOUCH bound of round 5: (W - 1) x touch2_hub <= 0.165, touch2_hub = the hubs' part of
        // sum_v (p_v + 5 q_v)^2 (p = token share: the context; q = unigram^0.75 share: the five negatives) -- minus the 40 / active a table of equally frequent
        // rows has, so that SBM graphs stay on the rho rule they were validated on.  What round 6 found out about it (profiles/r06_*.jsonl):
        //  * the bound was fitted through launches whose gaps were dominated by a HEAVY TAIL that has nothing to do with hubs: an isolated edge trained by two
        //    wavefronts at once (LOCALLY HOT ROWS, sgns_api.hip build_hotkey -- now handled; launches at one width agree to 0.2 % where they scattered over 6 %);
        //  * the staleness of the hubs' gradients is not the cause either: instrumented (GEMHIP_SGNS_STALENESS), the top hub's row takes 22 foreign updates
        //    between a wavefront's read and its add at 768 wavefronts; fresh reads / returning atomics cut that to 6 and the gap does not move; making every
        //    Hogwild write a lossless add makes it slightly WORSE; lowering the hot-row threshold 2-16x makes it worse and slower;
        //  * what is left is smooth in the width and larger on the larger graph -- R-MAT scale 17: -0.45 / -1.6 / -1.8 % at 256 / 768 / 1 536 wavefronts, scale 20:
        //    -1.3 / -3.0 / -6.0 % (paired with the sequential oracle, s.e. 0.3-0.5 %, 2-4 launches each) -- carried by query nodes of 1 000..30 000 tokens, and
        //    slower launches of the same configuration are the worse ones (queueing of the hot rows' atomic adds at the memory side is the suspect).
        // So the bound stays as the conservative extrapolation it is (548 wavefronts on scale 22 -- both oracle runs exist since round 6, their scoring did not finish: no pin yet), with a
        // FLOOR of 256 wavefronts: at 256 both measured graphs are at or inside -1.3 % (round 5's 50 wavefronts on scale 17 bought nothing for 3.5x the time:
        // ADVICE r5), and ONE bound for both unigram-table layouts -- round 5 halved it for the node-id layout on the strength of two launches (-6.3 % at 207
        // wavefronts) that the heavy tail explains; after the fix the layouts measure alike (scale 20, 768 wavefronts: -2.7 / -3.3 % and -2.5 / -4.3 %).
        const double touch_bound = 0.165;
        const double touch2_hub = std::max(0.0, vs.touch2 - 40.0 / std::max(1.0, vs.active > 0.0 ? vs.active : (double)n));
        const int64_t w_touch = touch2_hub > 0.0 ? std::max<int64_t>(256, 1 + (int64_t)std::min(1e15, touch_bound / (touch2_hub * kn.touch_scale))) : INT64_MAX;
        auto width = [&](bool all_cached) -> int64_t {
            // registers: the single-GPU kernels allocate 176-184 VGPRs (2 wavefronts per SIMD = 8 per CU), the bucket kernels 136-145 (3 per SIMD = 12 per CU)
            const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(kn.part ? 12 : 8, (int64_t)(160 * 1024) / (int64_t)(lds_bytes(P.delta, all_cached) + 512)));
            const int64_t w_dev = std::min<int64_t>(256 * per_cu, nwalks);
            const double w_steps = w_steps_of(all_cached);
            const bool reload_eff = w_steps < 1.0;
            int64_t hog_rho = std::max<int64_t>(1, (int64_t)(0.015 * n_eff / (5.0 * w_steps * kn.duty)));
            // hot rows: with W wavefronts the nodes with count >= tokens / ((W-1)(2R+1)) stay out of the LDS windows and take their negative updates
            // by atomic add (sgns_win_kernel), so the rule only has to hold over the remaining (cold) rows: the largest W that satisfies it
            if (reload_eff && kn.hot_count < 0 && n >= 8192 && hog_rho < std::min(std::min(w_dev, w_act), w_touch) && vs.total > 0.0) {
                for (int64_t wtry = std::min(std::min(w_dev, w_act), w_touch); wtry > hog_rho; wtry = wtry * 7 / 8) {
                    const double thr = std::max(2.0, std::ceil(vs.total / ((double)(wtry - 1) * span)));
                    if (0.015 * vs.n_eff_cold(thr) / (5.0 * w_steps * kn.duty) >= (double)wtry) { hog_rho = wtry; break; }
                }
            }
            const int64_t hog_win = kn.max_waves > 0 ? kn.max_waves : n >= 8192 ? std::min(hog_rho, w_touch) : std::min(hog_rho, hog_tiny);
            int64_t w = std::min<int64_t>(hog_win, w_dev);
            // Speed only (round 5): hot rows are updated by atomic adds at the memory side, and those saturate long before the device's wavefront slots do:
            // past ~three wavefronts per CU more wavefronts only queue up behind the same rows and touch them more often at once.  Measured per SGNS launch,
            // same box each (profiles/r05_rmat22_width_sweep.jsonl, r05_rmat20_width_sweep.jsonl): R-MAT scale 22 41.3 / 33.0 / 34.3 / 36.7 s and scale 20
            // 12.5 / 10.3 / 10.7 / 15.0 s at 512 / 768 / 1024 / 1536 wavefronts.  (A rate model -- min(W / wave step, atomic row operations per second / hot
            // operations per pair) -- fitted scale 22 and 17 and then put scale 20 at 496 wavefronts, 25 % slower than 768: the atomic unit's rate is not a
            // constant of the device, it grows with the number of distinct hot rows.  Dropped for the plain cap.)  Widths only ever shrink here.
            if (kn.max_waves == 0 && !kn.part && reload_eff && kn.hot_count < 0 && n >= 8192 && w > 768 && vs.total > 0.0 &&
                vs.max >= std::max(2.0, std::ceil(vs.total / ((double)(w - 1) * span))))
                w = 768;
            return w;
        };
        // the launch without the staging row holds one more wavefront per CU at d = 128 -- but only exists when no row is hot AT THAT WIDTH
        P.waves = width(allc);
        if (allc && hot_threshold(P.waves) != 0) { allc = false; P.waves = width(false); }
        if (P.waves == 1 && mode < 0) P.delta = false;
    }
    P.hot_thr = hot_threshold(P.waves);
    if (P.hot_thr == 0 && kn.has_local_hot && P.delta && P.waves > 1) P.hot_thr = INT32_MAX;       // only the locally hot nodes (hotkey INT32_MAX) qualify
    // (the launcher takes an ALLC instantiation iff R >= window && hot_thr == 0: `allc` false with hot_thr 0 only gives that kernel a row it does not use)
    P.lds = lds_bytes(P.delta, allc && P.hot_thr == 0);
    P.blocks = (int)P.waves; P.threads = 64;
    return P;
}

// the launch rule of gemhip_sgns_train on the rows in play: the negative rows are those of partition word_part (n_eff of ITS restricted unigram
// distribution bounds the Hogwild width: rho = W x 5 x 0.4 / n_eff <= 1.5 %); hot rows are judged on the GLOBAL token counts (a hub sits in
// W x (2R+1) x count / tokens windows whatever partition it belongs to)
SgnsKnobs bucket_knobs(const SgnsKnobs &handle, const VocabStats &vs_word, const VocabStats &vs_all, int32_t parts, int32_t walk_len, int32_t window,
                       int32_t flags, bool node_id_layout, bool corpus_hotkey, VocabStats *vs_out)
{
    VocabStats &vs = *vs_out;
    vs = vs_word;
    vs.total = vs_all.total; vs.max = vs_all.max; vs.touch2 = vs_all.touch2;
    SgnsKnobs kn = handle;
    kn.prefetch = 2; kn.reload = 1; kn.part = true; kn.node_id_layout = node_id_layout;
    // Duty cycle.  The rule bounds the negative rows that are OPEN at any time (W x 5 x w of them).  A wavefront of a bucket launch spends only part of
    // its time in pair steps: per walk it has walk_len x (window + 1) x 0.95 / parts^2 pairs to train but still 2 x walk_len / parts rows (the contexts and
    // the centre words of its two partitions) to fetch and return, each an exposed round trip of ~0.7 pair steps.  With that fraction f of the time in
    // pair steps the same bound on open rows allows W / f wavefronts (f = 0.88 for one partition -- left at 1, the validated rule --, 0.65 at 4, 0.47 at 8).
    if (parts > 1) {
        const double pairs_pp = (double)walk_len * (window + 1) * 0.95 / ((double)parts * parts), rows_pp = 2.0 * walk_len / parts;
        kn.duty = pairs_pp / (pairs_pp + 0.7 * rows_pp);
        // the pairs a bucket launch trains all have their context in ONE partition and their negatives in ONE partition: a row of those partitions is touched
        // `parts` times as often per trained pair as in the whole corpus (sum over the partition's rows of (parts x load)^2 = parts x touch2), in the
        // fraction `duty` of the time
        kn.touch_scale = (double)parts * kn.duty;
        // from ~4 partitions on a walk's contexts of one partition fit the window's slots and stay cached for the WHOLE walk (sgns_win_kernel<PART>,
        // whole-walk mode): a node then sits in W x walk_len x count / tokens windows, which is what decides whether it is hot
        if (walk_len / parts <= 2 * std::min(window, 10) + 1) kn.window_span = walk_len;
    }
    kn.has_local_hot = !(flags & 4) && corpus_hotkey;       // LOCALLY HOT ROWS of the gathered corpus (gemhip_n2v_locally_hot_corpus)
    return kn;
}

// InitUnigramTable (ELF @0x40e520) on a count vector: count^0.75, Vose in fp64, stacks popped from the back.
bool vose_unigram(const int32_t *cnt, int64_t n, int64_t stride, std::vector<float> &Uf, std::vector<int32_t> &K, std::vector<double> *U64)
{
    std::vector<double> U(n);
    std::vector<int32_t> small, large;
    K.assign(n, 0);
    double total = 0.0;
    for (int64_t i = 0; i < n; ++i) { U[i] = std::pow((double)cnt[i * stride], 0.75); total += U[i]; }
    if (!(total > 0.0)) return false;
    for (int64_t i = 0; i < n; ++i) U[i] /= total;
    small.reserve(n); large.reserve(n);
    for (int64_t i = 0; i < n; ++i) {
        U[i] = U[i] * (double)n;
        if (U[i] < 1.0) small.push_back((int32_t)i); else large.push_back((int32_t)i);
    }
    while (!small.empty() && !large.empty()) {
        const int32_t s = small.back(); small.pop_back();
        const int32_t l = large.back(); large.pop_back();
        K[s] = l;
        U[l] = U[l] + U[s] - 1.0;
        if (U[l] < 1.0) small.push_back(l); else large.push_back(l);
    }
    for (int32_t s : small) U[s] = 1.0;
    for (int32_t l : large) U[l] = 1.0;
    if (U64) *U64 = U;
    Uf.resize(n);
    for (int64_t i = 0; i < n; ++i) Uf[i] = (float)U[i];
    return true;
}

int build_unigram_tables(const int32_t *cnt, int64_t n, const int32_t *order, int32_t parts, int32_t flags, UnigramTables &T)
{
    T.vs.build(cnt, n);
    T.part_off.assign(parts + 1, 0);
    T.vs_part.assign(parts, VocabStats());
    T.part_slots.assign(parts, 0);
    for (int32_t p = 0; p < parts; ++p) T.part_off[p + 1] = T.part_off[p] + (n - p + parts - 1) / parts;
    T.U.assign(n, 0.f); T.K.assign(n, 0);                      // rows that are no entry of a table are never drawn
    T.slot.clear();
    if (order) T.slot.assign(n, -1);
    std::vector<std::vector<int32_t>> L(parts);                // partition p's table entries, in table order
    T.n_vocab = 0;
    if (order) { while (T.n_vocab < n && cnt[order[T.n_vocab]] > 0) ++T.n_vocab; }     // the nodes that occur come first (a node occurs iff it has a first token iff its count > 0)
    else T.n_vocab = n;
    for (int64_t r = 0; r < T.n_vocab; ++r) { const int32_t v = order ? order[r] : (int32_t)r; L[v % parts].push_back(v); }
    std::vector<int32_t> cp;
    for (int32_t p = 0; p < parts; ++p) {
        const int64_t off = T.part_off[p], np = T.part_off[p + 1] - off, Np = (int64_t)L[p].size();
        if (Np == 0) return p;
        std::vector<int32_t> cr(Np), K; std::vector<float> Uf;
        for (int64_t r = 0; r < Np; ++r) cr[r] = cnt[L[p][r]];
        if (!vose_unigram(cr.data(), Np, 1, Uf, K)) return p;
        for (int64_t r = 0; r < Np; ++r) {
            const int32_t loc = L[p][r] / parts, ali = L[p][K[r]] / parts;
            T.U[off + loc] = Uf[r]; T.K[off + loc] = ali;
            if (order) T.slot[off + r] = (flags & 2) ? ali : loc;
        }
        T.part_slots[p] = Np;
        if (parts == 1) { T.vs_part[p] = T.vs; continue; }     // (the same rows: the same statistics)
        cp.resize(np);
        for (int64_t i = 0; i < np; ++i) cp[i] = cnt[p + i * parts];
        T.vs_part[p].build(cp.data(), np);
    }
    return -1;
}

}  // namespace gemhip
