// Stand-alone driver of gem_amd/csrc/gf_plan.hip (GF's host planning): plain C++, no HIP, no device.
//
//   gf_plan_driver digest
//       stdout: per case of the list below one line for the acceptance rule, one for the row plan and one per unit plan -- the counts and a 64-bit
//       FNV-1a digest of every plan array; committed as tests/golden/gf_plan_digest.txt (recorded from the planner code as it moved out of gf.hip,
//       before anything in it was shared: CHANGELOG.md).  Every edge list is generated here from a seed.
//   gf_plan_driver rows <in> <out>
//       in:  int64 n, m, row_begin, row_end, hub_edges (0: no hub rows), has_w; int32 src[m]; int32 dst[m]; float w[m] if has_w
//       out: int64 kind (GfPlanError::Kind), edge, first, last; if kind == 0: int64 nrows, nupd, nlevels; int32 rows[nrows]; int64 ptr[nrows + 1];
//            uint32 col[nupd]; float w[nupd]; int64 level_off[nlevels + 1]; int64 level_hubs[nlevels]; int64 level_maxlen[nlevels]
//       (tests/test_gf_plan.py re-derives them in numpy from the reference's visiting order)
//
// scripts/build_asan_gf_plan.sh runs the first form under AddressSanitizer and UBSan.
#include "../../gem_amd/csrc/gf_plan.hpp"
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <string>

using namespace gemhip;

namespace {

struct Edges { int64_t n = 0; std::vector<int32_t> src, dst; std::vector<float> w; };

template <typename T> uint64_t fnv(const std::vector<T> &v)
{
    uint64_t h = 1469598103934665603ull;
    const unsigned char *p = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

// only raw mt19937 words are used (no <random> distribution: those differ between standard libraries)
Edges random_edges(int64_t n, int64_t m, uint32_t seed, bool weighted, int skew = 1)
{
    std::mt19937 mt(seed);
    Edges E; E.n = n;
    for (int64_t e = 0; e < m; ++e) {
        uint32_t i = mt() % (uint32_t)n;
        for (int k = 1; k < skew; ++k) i = std::min<uint32_t>(i, mt() % (uint32_t)n);      // skew > 1: low ids are sources far more often (power law-like)
        E.src.push_back((int32_t)i); E.dst.push_back((int32_t)(mt() % (uint32_t)n));
        if (weighted) E.w.push_back(0.5f + (float)(mt() % 1000) / 8.0f);
    }
    return E;
}

Edges permuted(const Edges &E, const std::vector<int64_t> &perm)
{
    Edges R; R.n = E.n;
    for (int64_t e : perm) { R.src.push_back(E.src[e]); R.dst.push_back(E.dst[e]); if (!E.w.empty()) R.w.push_back(E.w[e]); }
    return R;
}

std::vector<int64_t> iota_perm(size_t m) { std::vector<int64_t> p(m); std::iota(p.begin(), p.end(), 0); return p; }

Edges shuffled(const Edges &E, uint32_t seed)
{
    std::mt19937 mt(seed);
    std::vector<int64_t> p = iota_perm(E.src.size());
    for (size_t i = p.size(); i > 1; --i) std::swap(p[i - 1], p[mt() % i]);
    return permuted(E, p);
}

// edges [a, b) grouped by source; the sources ascending, or in the order `rank` gives them (a node-insertion order other than by id, as karate's)
Edges grouped(const Edges &E, size_t a, size_t b, const std::vector<int32_t> *rank = nullptr)
{
    std::vector<int64_t> p;
    for (size_t e = a; e < b; ++e) p.push_back((int64_t)e);
    std::stable_sort(p.begin(), p.end(), [&](int64_t x, int64_t y) { return rank ? (*rank)[E.src[x]] < (*rank)[E.src[y]] : E.src[x] < E.src[y]; });
    return permuted(E, p);
}

Edges concat(const Edges &A, const Edges &B)
{
    Edges R = A;
    R.src.insert(R.src.end(), B.src.begin(), B.src.end()); R.dst.insert(R.dst.end(), B.dst.begin(), B.dst.end()); R.w.insert(R.w.end(), B.w.begin(), B.w.end());
    return R;
}

void print_error(const GfPlanError &err)
{
    static const char *names[] = {"ok", "edge_out_of_range", "partly_updated", "too_many_units"};
    printf("%s edge=%lld first=%lld last=%lld", names[err.kind], (long long)err.edge, (long long)err.first, (long long)err.last);
}

void print_arrays(const GfHostPlan &P)
{
    printf(" rows=%016llx ptr=%016llx col=%016llx w=%016llx level_off=%016llx", (unsigned long long)fnv(P.rows), (unsigned long long)fnv(P.ptr),
           (unsigned long long)fnv(P.col), (unsigned long long)fnv(P.w), (unsigned long long)fnv(P.level_off));
}

void run_case(const char *name, const Edges &E, int64_t row_begin, int64_t row_end, int64_t hub_edges)
{
    const int64_t m = (int64_t)E.src.size();
    const float *w = E.w.empty() ? nullptr : E.w.data();
    printf("%s: n=%lld m=%lld order: ", name, (long long)E.n, (long long)m);
    print_error(gf_check_row_order(E.n, m, E.src.data(), E.dst.data()));
    printf("\n%s: rows [%lld,%lld) hub_edges=%lld: ", name, (long long)row_begin, (long long)row_end, (long long)hub_edges);
    GfHostPlan P;
    if (const GfPlanError err = gf_plan_rows(E.n, m, E.src.data(), E.dst.data(), w, row_begin, row_end, hub_edges, P)) print_error(err);
    else {
        int64_t hubs = 0, hub_levels = 0;
        for (int64_t h : P.level_hubs) { hubs += h; hub_levels += h > 0; }
        printf("rows=%lld nupd=%lld levels=%zu hubs=%lld in %lld levels hubs/level=[", (long long)P.nrows, (long long)P.nupd, P.level_hubs.size(), (long long)hubs,
               (long long)hub_levels);
        for (size_t l = 0; l < P.level_hubs.size() && l < 8; ++l) printf("%s%lld", l ? "," : "", (long long)P.level_hubs[l]);
        printf("%s] maxlen=[", P.level_hubs.size() > 8 ? ",.." : "");
        for (size_t l = 0; l < P.level_maxlen.size() && l < 8; ++l) printf("%s%lld", l ? "," : "", (long long)P.level_maxlen[l]);
        printf("%s]", P.level_maxlen.size() > 8 ? ",.." : "");
        print_arrays(P);
        printf(" level_hubs=%016llx level_maxlen=%016llx", (unsigned long long)fnv(P.level_hubs), (unsigned long long)fnv(P.level_maxlen));
    }
    printf("\n");
    for (int fused : {0, 1, 16}) {
        printf("%s: units fused_levels=%d: ", name, fused);
        GfHostPlan U;
        if (const GfPlanError err = gf_plan_units(E.n, m, E.src.data(), E.dst.data(), w, fused, U)) print_error(err);
        else {
            std::vector<int32_t> flat;
            int64_t nfused = 0;
            for (const GfSeg &g : U.segs) { flat.push_back(g.l0); flat.push_back(g.l1); flat.push_back(g.fused); nfused += g.fused; }
            printf("units=%lld nupd=%lld levels=%zu segments=%zu fused=%lld", (long long)U.nrows, (long long)U.nupd, U.level_off.size() - 1, U.segs.size(), (long long)nfused);
            print_arrays(U);
            printf(" segs=%016llx", (unsigned long long)fnv(flat));
        }
        printf("\n");
    }
}

int run_digest()
{
    const int64_t HUB = 1024;                                    // the library's default threshold
    const Edges karate = random_edges(34, 156, 1, false), g1k = random_edges(1000, 8000, 2, true);
    run_case("grouped-ascending", grouped(g1k, 0, g1k.src.size()), 0, 1000, HUB);
    run_case("karate-sized-shuffled", shuffled(karate, 11), 0, 34, HUB);
    run_case("1k-shuffled", shuffled(g1k, 12), 0, 1000, HUB);
    {   // sources grouped, but first visited in a scrambled order: the multi-level row plan (what karate's node order gives)
        std::vector<int32_t> rank(34);
        std::iota(rank.begin(), rank.end(), 0);
        std::mt19937 mt(5);
        for (size_t i = rank.size(); i > 1; --i) std::swap(rank[i - 1], rank[mt() % i]);
        run_case("karate-sized-insertion-order", grouped(karate, 0, karate.src.size(), &rank), 0, 34, HUB);
    }
    run_case("two-sorted-halves", concat(grouped(g1k, 0, 4000), grouped(g1k, 4000, 8000)), 0, 1000, HUB);
    {   // every edge of the first 50 once more, 7000 positions later
        Edges D = grouped(g1k, 0, g1k.src.size());
        Edges head; head.n = D.n;
        head.src.assign(D.src.begin(), D.src.begin() + 50); head.dst.assign(D.dst.begin(), D.dst.begin() + 50); head.w.assign(D.w.begin(), D.w.begin() + 50);
        run_case("duplicates-far-apart", concat(D, head), 0, 1000, HUB);
    }
    {   // self-loops and edges that do not fire (dst <= src) between firing ones
        Edges S; S.n = 8;
        const int32_t e[][2] = {{0, 0}, {0, 3}, {3, 0}, {1, 1}, {1, 2}, {2, 1}, {2, 5}, {5, 5}, {7, 2}, {4, 6}, {6, 4}, {6, 7}};
        for (const auto &p : e) { S.src.push_back(p[0]); S.dst.push_back(p[1]); }
        run_case("self-loops-and-non-firing", S, 0, 8, HUB);
    }
    {
        Edges R; R.n = 4; R.src = {1, 0, 1}; R.dst = {2, 1, 3};
        run_case("refusal-list", R, 0, 4, HUB);
        Edges O = R; O.dst[2] = 4;
        run_case("endpoint-out-of-range", O, 0, 4, HUB);
        Edges Z; Z.n = 5;
        run_case("m=0", Z, 0, 5, HUB);
    }
    run_case("row-range-inside", grouped(g1k, 0, g1k.src.size()), 250, 700, HUB);
    {   // power law-like sources, first visited in a scrambled order, hub threshold 8: levels with and without hub rows
        const Edges pl = random_edges(4000, 12000, 3, true, 2);
        std::vector<int32_t> rank(4000);
        std::iota(rank.begin(), rank.end(), 0);
        std::mt19937 mt(6);
        for (size_t i = rank.size(); i > 1; --i) std::swap(rank[i - 1], rank[mt() % i]);
        const Edges G = grouped(pl, 0, pl.src.size(), &rank);
        run_case("power-law-hub8", G, 0, 4000, 8);
        run_case("power-law-no-hubs", G, 0, 4000, 0);
    }
    for (int forced : {0, 3})
        for (int64_t maxlen : {0, 128, 129})
            for (int64_t nrows : {0, 16383, 16384, 32768, 946188, 100000000})
                printf("rows_per_wave forced=%d maxlen=%lld nrows=%lld: %d %d\n", forced, (long long)maxlen, (long long)nrows,
                       gf_level_rows_per_wave(forced, maxlen, nrows, 8), gf_level_rows_per_wave(forced, maxlen, nrows, 64));
    fflush(stdout);
    return 0;
}

int run_rows_file(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb");
    int64_t hdr[6];
    if (!f || fread(hdr, 8, 6, f) != 6 || hdr[0] < 1 || hdr[1] < 0) { fprintf(stderr, "gf_plan_driver: bad input %s\n", in_path); return 2; }
    const int64_t n = hdr[0], m = hdr[1];
    std::vector<int32_t> src(m), dst(m);
    std::vector<float> w(hdr[5] ? m : 0);
    if (fread(src.data(), 4, m, f) != (size_t)m || fread(dst.data(), 4, m, f) != (size_t)m || fread(w.data(), 4, w.size(), f) != w.size()) {
        fprintf(stderr, "gf_plan_driver: short input %s\n", in_path);
        return 2;
    }
    fclose(f);
    GfHostPlan P;
    const GfPlanError err = gf_plan_rows(n, m, src.data(), dst.data(), hdr[5] ? w.data() : nullptr, hdr[2], hdr[3], hdr[4], P);
    FILE *o = fopen(out_path, "wb");
    if (!o) { fprintf(stderr, "gf_plan_driver: cannot write %s\n", out_path); return 2; }
    const int64_t head[4] = {(int64_t)err.kind, err.edge, err.first, err.last};
    fwrite(head, 8, 4, o);
    if (!err) {
        const int64_t counts[3] = {P.nrows, P.nupd, (int64_t)P.level_hubs.size()};
        fwrite(counts, 8, 3, o);
        fwrite(P.rows.data(), 4, P.rows.size(), o); fwrite(P.ptr.data(), 8, P.ptr.size(), o);
        fwrite(P.col.data(), 4, P.col.size(), o); fwrite(P.w.data(), 4, P.w.size(), o);
        fwrite(P.level_off.data(), 8, P.level_off.size(), o); fwrite(P.level_hubs.data(), 8, P.level_hubs.size(), o);
        fwrite(P.level_maxlen.data(), 8, P.level_maxlen.size(), o);
    }
    return fclose(o) ? 2 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "digest")) return run_digest();
    if (argc == 4 && !strcmp(argv[1], "rows")) return run_rows_file(argv[2], argv[3]);
    fprintf(stderr, "usage: %s digest | rows <in> <out>\n", argv[0]);
    return 2;
}
