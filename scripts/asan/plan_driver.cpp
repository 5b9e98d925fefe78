// Stand-alone driver of gem_amd/csrc/sgns_plan.hip (the SGNS launch rule and the unigram tables): plain C++, no HIP, no device.
//
//   plan_driver grid <tests/golden/rmat_token_count_histograms.json>
//       stdout: one line per case of the launch-rule grid below -- `window delta R waves hot_thr lds blocks threads` after the case's name; it is
//       committed as tests/golden/sgns_plan_grid.txt (recorded from the arithmetic BEFORE the rule moved into sgns_plan.hip: CHANGELOG.md).
//       Then the unified table builder on small inputs, its invariants checked; stderr: a summary.  Exit status 1 when an invariant fails.
//   plan_driver tables <in> <out>
//       in:  int32 n, parts, flags, has_order; int32 counts[n]; int32 order[n] if has_order
//       out: int32 rc; int64 n_vocab; float U[n]; int32 K[n]; int32 slot[n] (all -1 in the node-id layout); int64 part_off[parts + 1]; int64 part_slots[parts]
//       (tests/test_sgns_plan.py compares them with the oracle's tables, bit for bit)
//
// scripts/build_asan_plan.sh runs the first form under AddressSanitizer and UBSan.
#include "../../gem_amd/csrc/sgns_plan.hpp"
#include "../../include/gem_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

using namespace gemhip;

namespace {

struct Counts { std::string name; std::vector<int32_t> c; int64_t nwalks_big; };

// zipf_counts of tests/test_sgns_plan.py: ranks = RandomState(seed).permutation(n) + 1 (MT19937 seeded with the integer; the legacy shuffle: for i = n-1 .. 1
// swap with a masked-rejection draw from [0, i]), count = max(1, round(tokens x rank^-s / sum))
std::vector<int32_t> zipf_counts(int64_t n, double tokens, double s, uint32_t seed)
{
    std::mt19937 mt(seed);
    std::vector<int64_t> perm(n);
    for (int64_t i = 0; i < n; ++i) perm[i] = i;
    for (int64_t i = n - 1; i >= 1; --i) {
        uint32_t mask = (uint32_t)i;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        uint32_t j;
        do j = (uint32_t)mt() & mask; while (j > (uint32_t)i);
        std::swap(perm[i], perm[j]);
    }
    std::vector<double> c(n);
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) { c[i] = 1.0 / std::pow((double)perm[i] + 1.0, s); sum += c[i]; }
    std::vector<int32_t> out(n);
    for (int64_t i = 0; i < n; ++i) out[i] = (int32_t)std::max(1.0, std::nearbyint(c[i] / sum * tokens));
    return out;
}

// {"<name>": {"n": .., "nwalks": .., "count": [..], "nodes": [..], ..}, ..}: nodes[i] nodes have count[i] tokens, the other n - sum(nodes) none
bool read_histogram(const std::string &json, const char *name, Counts &out)
{
    const size_t at = json.find(std::string("\"") + name + "\"");
    if (at == std::string::npos) return false;
    auto number = [&](const char *key) -> int64_t {
        const size_t k = json.find(std::string("\"") + key + "\":", at);
        return k == std::string::npos ? -1 : strtoll(json.c_str() + k + strlen(key) + 3, nullptr, 10);
    };
    auto list = [&](const char *key) {
        std::vector<int64_t> v;
        size_t k = json.find(std::string("\"") + key + "\": [", at);
        if (k == std::string::npos) return v;
        const char *p = json.c_str() + k + strlen(key) + 5;
        for (;;) {
            char *e;
            v.push_back(strtoll(p, &e, 10));
            p = e;
            while (*p == ' ' || *p == ',') ++p;
            if (*p == ']' || *p == 0) break;
        }
        return v;
    };
    const int64_t n = number("n");
    const std::vector<int64_t> count = list("count"), nodes = list("nodes");
    if (n <= 0 || count.empty() || count.size() != nodes.size()) return false;
    out.name = name; out.nwalks_big = number("nwalks"); out.c.clear();
    for (size_t i = 0; i < count.size(); ++i) out.c.insert(out.c.end(), (size_t)nodes[i], (int32_t)count[i]);
    if ((int64_t)out.c.size() > n) return false;
    out.c.resize(n, 0);
    return true;
}

void print_plan(const std::string &name, const SgnsLaunchPlan &P)
{
    printf("%s: %d %d %d %lld %d %zu %d %d\n", name.c_str(), (int)P.window, (int)P.delta, P.R, (long long)P.waves, (int)P.hot_thr, P.lds, P.blocks, P.threads);
}

struct Variant { const char *name; SgnsKnobs kn; };

int run_grid(const char *hist_path)
{
    std::string json;
    if (FILE *f = fopen(hist_path, "rb")) {
        char buf[65536]; size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) json.append(buf, got);
        fclose(f);
    } else { fprintf(stderr, "plan_driver: cannot read %s\n", hist_path); return 2; }

    std::vector<Counts> V;
    for (int64_t n : {1024, 4096, 8192, 100000}) V.push_back({"uniform" + std::to_string(n), std::vector<int32_t>(n, 800), 10 * n});
    V.push_back({"zipf0.6", zipf_counts(131072, 131072.0 * 800, 0.6, 0), 10 * 131072});
    V.push_back({"zipf1.0", zipf_counts(131072, 131072.0 * 800, 1.0, 0), 10 * 131072});
    { Counts h{"halfempty", std::vector<int32_t>(200000, 0), 1000000}; for (size_t i = 0; i < h.c.size(); i += 2) h.c[i] = 800; V.push_back(h); }
    for (const char *name : {"rmat17", "rmat20", "rmat22"}) {
        Counts h;
        if (!read_histogram(json, name, h)) { fprintf(stderr, "plan_driver: no histogram %s in %s\n", name, hist_path); return 2; }
        V.push_back(h);
    }
    std::vector<VocabStats> S(V.size());
    for (size_t i = 0; i < V.size(); ++i) S[i].build(V[i].c.data(), (int64_t)V[i].c.size());

    const int all_d[] = {16, 64, 127, 128, 129, 182, 256, 384}, windows[] = {5, 10, 12}, walk_lens[] = {2, 80};
    const int all_flags[] = {11, 27, 11 | 4, 27 | 4, 11 | GEMHIP_N2V_NO_WINDOW_CACHE};
    auto nwalks_of = [&](const Counts &v, int k) -> int64_t { return k ? v.nwalks_big : 100; };     // above / below the device's width (256 CUs x 7 wavefronts)
    auto case_name = [](const Counts &v, const char *variant, int d, int w, int l, int64_t nw, int flags) {
        char b[256];                                           // <counts> <knobs> d window walk_len nwalks flags
        snprintf(b, sizeof b, "%s %s %d %d %d %lld %d", v.name.c_str(), variant, d, w, l, (long long)nw, flags);
        return std::string(b);
    };

    auto by_name = [&](std::initializer_list<const char *> names) {
        std::vector<size_t> idx;
        for (const char *nm : names) for (size_t i = 0; i < V.size(); ++i) if (V[i].name == nm) idx.push_back(i);
        return idx;
    };
    auto emit = [&](size_t i, const char *variant, SgnsKnobs kn, int d, int w, int l, int k, int flags) {
        kn.node_id_layout = !(flags & GEMHIP_N2V_VOCAB_ORDER);
        const int64_t nw = nwalks_of(V[i], k);
        print_plan(case_name(V[i], variant, d, w, l, nw, flags), plan_sgns_launch(S[i], kn, (int64_t)V[i].c.size(), d, w, l, nw, flags));
    };
    // Not the full cross (it is ~10 000 lines): each block crosses the inputs that meet in one part of the rule.
    // 1. the width rule proper -- vocabulary x row width x window -- on the plugin's launch (flags 27, walk_len 80, more walks than wavefronts)
    for (size_t i = 0; i < V.size(); ++i)
        for (int d : all_d) for (int w : windows) emit(i, "default", SgnsKnobs(), d, w, 80, 1, 27);
    // 2. what gates the kernel and caps the width whatever the vocabulary: flags, walk_len, nwalks -- without hubs below / above 8192 nodes and with hubs,
    //    at one LDS row per embedding row (128), the first width on the four-chunk kernel (129) and rows too wide for the window (384)
    for (size_t i : by_name({"uniform1024", "uniform100000", "rmat17"}))
        for (int d : {128, 129, 384}) for (int l : walk_lens) for (int k = 0; k < 2; ++k) for (int flags : all_flags)
            emit(i, "default", SgnsKnobs(), d, 10, l, k, flags);
    // 3. one knob off its default at a time, Hogwild and deterministic
    std::vector<Variant> variants;
    auto add = [&](const char *name, void (*set)(SgnsKnobs &)) { Variant v{name, SgnsKnobs()}; set(v.kn); variants.push_back(v); };
    add("max_waves=1", [](SgnsKnobs &k) { k.max_waves = 1; });
    add("max_waves=8", [](SgnsKnobs &k) { k.max_waves = 8; });
    add("cache_radius=0", [](SgnsKnobs &k) { k.cache_radius = 0; });
    add("cache_radius=3", [](SgnsKnobs &k) { k.cache_radius = 3; });
    add("cache_delta=0", [](SgnsKnobs &k) { k.cache_delta = 0; });
    add("cache_delta=1", [](SgnsKnobs &k) { k.cache_delta = 1; });
    add("hot_count=0", [](SgnsKnobs &k) { k.hot_count = 0; });
    add("hot_count=50", [](SgnsKnobs &k) { k.hot_count = 50; });
    add("has_local_hot", [](SgnsKnobs &k) { k.has_local_hot = true; });
    const std::vector<size_t> five = by_name({"uniform8192", "uniform100000", "zipf1.0", "halfempty", "rmat17"});
    for (const Variant &var : variants)
        for (size_t i : five) for (int d : {128, 129}) for (int flags : {11, 11 | 4}) emit(i, var.name, var.kn, d, 10, 80, 1, flags);
    // 4. the A/B shape of the benchmark: prefetch distance 1 without reload-on-update exists at d = 128 with the whole window cached (window <= 10)
    for (size_t i = 0; i < V.size(); ++i)
        for (int w : windows) for (int flags : {11, 11 | 4}) {
            SgnsKnobs kn; kn.prefetch = 1; kn.reload = 0;
            emit(i, "prefetch=1,reload=0", kn, 128, w, 80, 1, flags);
        }
    // 5. bucket launches of the partitioned schedule: partition 0 of `parts`; Hogwild without / with a hot key of the gathered corpus, and deterministic
    for (size_t i : five)
        for (int parts : {1, 2, 4, 8}) {
            std::vector<int32_t> cp;
            for (size_t v = 0; v < V[i].c.size(); v += parts) cp.push_back(V[i].c[v]);
            VocabStats sp; sp.build(cp.data(), (int64_t)cp.size());
            for (int w : {10}) for (int l : walk_lens) for (int c = 0; c < 3; ++c) {
                const int flags = c == 2 ? 27 | 4 : 27, hot = c == 1;
                VocabStats vs;
                const SgnsKnobs kn = bucket_knobs(SgnsKnobs(), sp, S[i], parts, l, w, flags, false, hot != 0, &vs);
                char var[128];
                snprintf(var, sizeof var, "bucket,parts=%d,hotkey=%d,duty=%.17g,touch_scale=%.17g,span=%d", parts, hot, kn.duty, kn.touch_scale, (int)kn.window_span);
                print_plan(case_name(V[i], var, 128, w, l, V[i].nwalks_big, flags), plan_sgns_launch(vs, kn, (int64_t)cp.size(), 128, w, l, V[i].nwalks_big, flags));
            }
        }
    fflush(stdout);
    return 0;
}

// ---- the unified table builder on small inputs
int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

// one build, in the node-id layout (order empty) or the binary's: every invariant that does not need an oracle
void check_tables(const char *what, const std::vector<int32_t> &cnt, const std::vector<int32_t> &order, int parts, int flags)
{
    const int64_t n = (int64_t)cnt.size();
    int want_rc = -1;                                          // refused with the first partition none of whose nodes occurs
    for (int p = parts - 1; p >= 0; --p) {
        bool any = false;
        for (int64_t v = p; v < n; v += parts) any = any || cnt[v] > 0;
        if (!any) want_rc = p;
    }
    UnigramTables T;
    const int rc = build_unigram_tables(cnt.data(), n, order.empty() ? nullptr : order.data(), parts, flags, T);
    EXPECT(rc == want_rc, "%s: n=%lld parts=%d: rc %d, expected %d", what, (long long)n, parts, rc, want_rc);
    if (rc >= 0 || want_rc >= 0) return;
    EXPECT((int64_t)T.U.size() == n && (int64_t)T.K.size() == n && T.part_off.back() == n, "%s: sizes", what);
    int64_t slots = 0;
    for (int p = 0; p < parts; ++p) {
        const int64_t off = T.part_off[p], np = T.part_off[p + 1] - off;
        EXPECT(np == (n - p + parts - 1) / parts, "%s: partition %d has %lld rows", what, p, (long long)np);
        // the partition's entries in table order, and Vose over them in fp64
        std::vector<int32_t> rows, cr;
        if (order.empty()) for (int64_t v = p; v < n; v += parts) rows.push_back((int32_t)v);
        else for (int64_t r = 0; r < n && cnt[order[r]] > 0; ++r) if (order[r] % parts == p) rows.push_back(order[r]);
        for (int32_t v : rows) cr.push_back(cnt[v]);
        EXPECT(T.part_slots[p] == (int64_t)rows.size(), "%s: partition %d: %lld slots for %zu entries", what, p, (long long)T.part_slots[p], rows.size());
        slots += T.part_slots[p];
        std::vector<float> Uf; std::vector<int32_t> K; std::vector<double> U;
        EXPECT(vose_unigram(cr.data(), (int64_t)cr.size(), 1, Uf, K, &U), "%s: partition %d: Vose", what, p);
        double Z = 0.0;
        for (int32_t c : cr) Z += std::pow((double)c, 0.75);
        const double N = (double)cr.size();
        std::vector<double> mass(cr.size(), 0.0);           // what the alias table draws: slot r with U[r] / N, its alias with the rest
        for (size_t r = 0; r < cr.size(); ++r) {
            EXPECT(U[r] >= 0.0 && U[r] <= 1.0 && Uf[r] >= 0.f && Uf[r] <= 1.f, "%s: partition %d: U[%zu] = %.17g", what, p, r, U[r]);
            EXPECT(K[r] >= 0 && K[r] < (int32_t)cr.size(), "%s: partition %d: K[%zu] = %d", what, p, r, K[r]);
            mass[r] += U[r] / N; mass[K[r]] += (1.0 - U[r]) / N;
        }
        for (size_t r = 0; r < cr.size(); ++r)
            EXPECT(std::fabs(mass[r] - std::pow((double)cr[r], 0.75) / Z) <= 1e-12, "%s: partition %d: entry %zu drawn with %.17g, count^0.75 / Z = %.17g", what, p, r, mass[r],
                   std::pow((double)cr[r], 0.75) / Z);
        // ... and the builder's arrays are that table by local row, aliases inside the partition
        for (size_t r = 0; r < rows.size(); ++r) {
            const int64_t loc = rows[r] / parts, ali = rows[K[r]] / parts;
            EXPECT(memcmp(&T.U[off + loc], &Uf[r], 4) == 0 && T.K[off + loc] == ali, "%s: partition %d: row %lld", what, p, (long long)loc);
            EXPECT(T.K[off + loc] >= 0 && T.K[off + loc] < np, "%s: partition %d: alias of row %lld outside the partition", what, p, (long long)loc);
            if (!order.empty()) EXPECT(T.slot[off + r] == ((flags & 2) ? ali : loc), "%s: partition %d: slot %zu", what, p, r);
        }
        if (!order.empty()) for (int64_t s = (int64_t)rows.size(); s < np; ++s) EXPECT(T.slot[off + s] == -1, "%s: partition %d: slot %lld beyond the slot count", what, p, (long long)s);
        EXPECT(T.vs_part[p].n == (double)np, "%s: partition %d: statistics over %g rows", what, p, T.vs_part[p].n);
    }
    EXPECT(T.n_vocab == slots, "%s: n_vocab %lld, slots %lld", what, (long long)T.n_vocab, (long long)slots);
    int64_t active = 0;
    for (int32_t c : cnt) active += c > 0;
    EXPECT(T.vs.active == (double)active && T.vs.n == (double)n, "%s: global statistics", what);
    if (!order.empty()) EXPECT(T.n_vocab == active, "%s: %lld slots, %lld nodes occur", what, (long long)T.n_vocab, (long long)active);
}

// a first-appearance order for counts: the nodes that occur in a scrambled but fixed order, the others after them
std::vector<int32_t> some_order(const std::vector<int32_t> &cnt)
{
    std::vector<int32_t> occ, rest;
    for (size_t v = 0; v < cnt.size(); ++v) (cnt[v] > 0 ? occ : rest).push_back((int32_t)v);
    std::mt19937 mt(7);
    for (size_t i = occ.size(); i > 1; --i) std::swap(occ[i - 1], occ[mt() % i]);
    occ.insert(occ.end(), rest.begin(), rest.end());
    return occ;
}

int run_table_cases()
{
    int cases = 0;
    std::mt19937 mt(1);
    for (int64_t n : {1, 2, 7, 1024})
        for (int parts : {1, 2, 4}) {
            if (parts > n) continue;
            std::vector<int32_t> cnt(n);
            for (auto &c : cnt) c = 1 + (int32_t)(mt() % 1000) * (int32_t)(mt() % 3);         // every node occurs; a third of them once
            for (int flags : {11, 9}) {
                check_tables("every node occurs", cnt, {}, parts, flags);
                check_tables("every node occurs", cnt, some_order(cnt), parts, flags);
                cases += 2;
            }
            if (n < 7) continue;
            // nodes that never occur (7 = 4 + 3: the strided partitions' last slices are one element short of the first's)
            std::vector<int32_t> holes(cnt);
            for (int64_t v = 0; v < n; v += 3) holes[v] = 0;
            check_tables("a third never occurs", holes, {}, parts, 11);
            check_tables("a third never occurs", holes, some_order(holes), parts, 11);
            cases += 2;
            // a partition with no occurring node (n = 7 in four partitions above was one already): refused, and named
            if (parts > 1) {
                std::vector<int32_t> gone(cnt);
                for (int64_t v = parts - 1; v < n; v += parts) gone[v] = 0;
                check_tables("the last partition never occurs", gone, {}, parts, 11);
                check_tables("the last partition never occurs", gone, some_order(gone), parts, 11);
                cases += 2;
            }
            // all-zero counts: the empty vocabulary
            const std::vector<int32_t> zero(n, 0);
            check_tables("no node occurs", zero, {}, parts, 11);
            check_tables("no node occurs", zero, some_order(zero), parts, 11);
            UnigramTables T;
            const std::vector<int32_t> ord = some_order(zero);
            build_unigram_tables(zero.data(), n, ord.data(), parts, 11, T);
            EXPECT(T.n_vocab == 0, "no node occurs: n_vocab %lld", (long long)T.n_vocab);
            cases += 4;
        }
    fprintf(stderr, "table builder: %d cases, %d failed checks\n", cases, failures);
    return failures ? 1 : 0;
}

int run_tables_file(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb");
    int32_t hdr[4];
    if (!f || fread(hdr, 4, 4, f) != 4 || hdr[0] < 1 || hdr[1] < 1) { fprintf(stderr, "plan_driver: bad input %s\n", in_path); return 2; }
    const int64_t n = hdr[0];
    std::vector<int32_t> cnt(n), order(hdr[3] ? n : 0);
    if (fread(cnt.data(), 4, n, f) != (size_t)n || (hdr[3] && fread(order.data(), 4, n, f) != (size_t)n)) { fprintf(stderr, "plan_driver: short input %s\n", in_path); return 2; }
    fclose(f);
    UnigramTables T;
    const int32_t rc = build_unigram_tables(cnt.data(), n, hdr[3] ? order.data() : nullptr, hdr[1], hdr[2], T);
    T.slot.resize(n, -1); T.part_slots.resize(hdr[1], 0);
    FILE *o = fopen(out_path, "wb");
    if (!o) { fprintf(stderr, "plan_driver: cannot write %s\n", out_path); return 2; }
    fwrite(&rc, 4, 1, o); fwrite(&T.n_vocab, 8, 1, o);
    fwrite(T.U.data(), 4, n, o); fwrite(T.K.data(), 4, n, o); fwrite(T.slot.data(), 4, n, o);
    fwrite(T.part_off.data(), 8, hdr[1] + 1, o); fwrite(T.part_slots.data(), 8, hdr[1], o);
    return fclose(o) ? 2 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "grid")) {
        if (int rc = run_grid(argv[2])) return rc;
        return run_table_cases();
    }
    if (argc == 4 && !strcmp(argv[1], "tables")) return run_tables_file(argv[2], argv[3]);
    fprintf(stderr, "usage: %s grid <rmat_token_count_histograms.json> | tables <in> <out>\n", argv[0]);
    return 2;
}
