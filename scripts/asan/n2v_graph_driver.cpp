// Stand-alone driver of gem_amd/csrc/n2v_graph.hip (what gemhip_n2v_create derives from a CSR; the renaming of the binary-layout unigram table) and of
// sgns_knobs_from_env (gem_amd/csrc/sgns_plan.hip): plain C++, no HIP, no device.
//
//   n2v_graph_driver graph <in> <out>
//       in:  int64 n, nnz, hub_deg, has_w, len_row_ptr, len_col; int64 row_ptr[len_row_ptr]; int32 col[len_col]; float w[len_col] if has_w
//            (len_row_ptr 0 / len_col 0 pass a null pointer)
//       out: int64 kind, index, column; and when kind == 0: int64 uniform, nstart, nhub, nw; int32 col[nnz]; float w[nw]; int32 start[nstart];
//            int32 hub_rows[nhub]; int64 hub_off[nhub ? nhub + 1 : size as built]
//   n2v_graph_driver rename <in> <out>
//       in:  int64 n, n_vocab; int32 back[n_vocab]; float U[n]; int32 K[n]        out: float UT[n_vocab]; int32 KT[n_vocab]
//   n2v_graph_driver knobs [NAME=VALUE ...]
//       stdout: max_waves cache_radius cache_delta prefetch reload hot_count local_hot fresh neg_count of sgns_knobs_from_env over exactly those variables
//   n2v_graph_driver self
//       the cases of tests/test_n2v_graph.py in miniature, checked against a restatement; exit status 1 when one fails
//
// tests/test_n2v_graph.py uses the first three forms; scripts/build_asan_n2v_graph.sh runs `self` under AddressSanitizer and UBSan.
#include "../../gem_amd/csrc/n2v_graph.hpp"
#include "../../gem_amd/csrc/sgns_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <utility>

using namespace gemhip;

namespace {

template <typename T> bool read_vec(FILE *f, std::vector<T> &v, int64_t count)
{
    v.resize((size_t)count);
    return count == 0 || fread(v.data(), sizeof(T), (size_t)count, f) == (size_t)count;
}
template <typename T> void write_vec(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

int run_graph(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb");
    int64_t hdr[6];
    std::vector<int64_t> rp; std::vector<int32_t> col; std::vector<float> w;
    if (!f || fread(hdr, 8, 6, f) != 6 || !read_vec(f, rp, hdr[4]) || !read_vec(f, col, hdr[5]) || !read_vec(f, w, hdr[3] ? hdr[5] : 0)) {
        fprintf(stderr, "n2v_graph_driver: bad input %s\n", in_path); return 2;
    }
    fclose(f);
    N2vGraph g;
    const N2vGraphError e = prepare_n2v_graph(hdr[0], hdr[1], rp.empty() ? nullptr : rp.data(), col.empty() ? nullptr : col.data(), hdr[3] ? w.data() : nullptr, g, (int)hdr[2]);
    FILE *o = fopen(out_path, "wb");
    if (!o) { fprintf(stderr, "n2v_graph_driver: cannot write %s\n", out_path); return 2; }
    const int64_t err[3] = {(int64_t)e.kind, e.index, (int64_t)e.column};
    fwrite(err, 8, 3, o);
    if (!e) {
        const int64_t sizes[4] = {(int64_t)g.uniform, (int64_t)g.start.size(), (int64_t)g.hub_rows.size(), (int64_t)g.w.size()};
        fwrite(sizes, 8, 4, o);
        write_vec(o, g.col); write_vec(o, g.w); write_vec(o, g.start); write_vec(o, g.hub_rows); write_vec(o, g.hub_off);
    }
    return fclose(o) ? 2 : 0;
}

int run_rename(const char *in_path, const char *out_path)
{
    FILE *f = fopen(in_path, "rb");
    int64_t hdr[2];
    std::vector<int32_t> back, K; std::vector<float> U;
    if (!f || fread(hdr, 8, 2, f) != 2 || !read_vec(f, back, hdr[1]) || !read_vec(f, U, hdr[0]) || !read_vec(f, K, hdr[0])) {
        fprintf(stderr, "n2v_graph_driver: bad input %s\n", in_path); return 2;
    }
    fclose(f);
    std::vector<float> UT((size_t)hdr[1]); std::vector<int32_t> KT((size_t)hdr[1]);
    unigram_table_renamed(hdr[0], hdr[1], back.data(), U.data(), K.data(), UT.data(), KT.data());
    FILE *o = fopen(out_path, "wb");
    if (!o) { fprintf(stderr, "n2v_graph_driver: cannot write %s\n", out_path); return 2; }
    write_vec(o, UT); write_vec(o, KT);
    return fclose(o) ? 2 : 0;
}

// the environment sgns_knobs_from_env is shown: NAME=VALUE strings, never the process's own
std::vector<std::string> fake_env;
const char *fake_lookup(const char *name)
{
    const size_t len = strlen(name);
    for (const std::string &s : fake_env) if (s.size() > len && s[len] == '=' && !s.compare(0, len, name)) return s.c_str() + len + 1;
    return nullptr;
}
std::vector<int> knob_values(const SgnsKnobs &k) { return {k.max_waves, k.cache_radius, k.cache_delta, k.prefetch, k.reload, k.hot_count, k.local_hot, k.fresh, k.neg_count}; }

int run_knobs(int argc, char **argv)
{
    fake_env.assign(argv, argv + argc);
    const std::vector<int> v = knob_values(sgns_knobs_from_env(fake_lookup));
    for (size_t i = 0; i < v.size(); ++i) printf("%s%d", i ? " " : "", v[i]);
    printf("\n");
    return 0;
}

// ---- self checks
int failures = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++failures; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Csr { int64_t n; std::vector<int64_t> rp; std::vector<int32_t> col; std::vector<float> w; };

// n rows of random degree below max_deg, columns in random order (repeats allowed), weights per edge or -- row_uniform -- one value per row
Csr random_csr(int64_t n, int max_deg, bool weighted, bool row_uniform, uint32_t seed)
{
    std::mt19937 mt(seed);
    Csr g{n, {0}, {}, {}};
    for (int64_t v = 0; v < n; ++v) {
        const int deg = (int)(mt() % (uint32_t)max_deg);
        const float wr = 0.5f + (float)(mt() % 7);
        for (int k = 0; k < deg; ++k) { g.col.push_back((int32_t)(mt() % (uint32_t)n)); if (weighted) g.w.push_back(row_uniform ? wr : 0.25f + (float)(mt() % 1000) / 100.f); }
        g.rp.push_back((int64_t)g.col.size());
    }
    return g;
}

// the edges grouped by source in list order (rows stay unsorted)
Csr csr_of_edges(int64_t n, const std::vector<int32_t> &src, const std::vector<int32_t> &dst)
{
    Csr g{n, {0}, {}, {}};
    for (int64_t v = 0; v < n; ++v) {
        for (size_t k = 0; k < src.size(); ++k) if (src[k] == v) g.col.push_back(dst[k]);
        g.rp.push_back((int64_t)g.col.size());
    }
    return g;
}

void check_graph(const char *what, const Csr &g, int hub_deg)
{
    N2vGraph out;
    const int64_t nnz = (int64_t)g.col.size();
    const N2vGraphError e = prepare_n2v_graph(g.n, nnz, g.rp.data(), g.col.data(), g.w.empty() ? nullptr : g.w.data(), out, hub_deg);
    EXPECT(!e, "%s: refused with kind %d at %lld", what, (int)e.kind, (long long)e.index);
    if (e) return;
    bool uniform = true;
    std::vector<char> present(g.n, 0);
    std::vector<int32_t> hubs; std::vector<int64_t> hoff{0};
    for (int64_t v = 0; v < g.n; ++v) {
        const int64_t a = g.rp[v], b = g.rp[v + 1];
        std::vector<std::pair<int32_t, int64_t>> key;          // (column, position): the stable order, restated as a total order
        for (int64_t k = a; k < b; ++k) { key.emplace_back(g.col[k], k); present[g.col[k]] = 1; present[v] = 1; if (!g.w.empty() && g.w[k] != g.w[a]) uniform = false; }
        std::sort(key.begin(), key.end());
        for (int64_t k = a; k < b; ++k) {
            EXPECT(out.col[k] == key[k - a].first, "%s: row %lld column %lld", what, (long long)v, (long long)(k - a));
            if (!g.w.empty()) EXPECT(memcmp(&out.w[k], &g.w[key[k - a].second], 4) == 0, "%s: row %lld weight %lld did not follow its column", what, (long long)v, (long long)(k - a));
        }
        if (b - a >= hub_deg) { hubs.push_back((int32_t)v); hoff.push_back(hoff.back() + (b - a)); }
    }
    EXPECT(out.uniform == uniform, "%s: uniform %d", what, (int)out.uniform);
    EXPECT(out.w.size() == g.w.size(), "%s: %zu weights", what, out.w.size());
    std::vector<int32_t> start;
    for (int64_t v = 0; v < g.n; ++v) if (present[v]) start.push_back((int32_t)v);
    EXPECT(out.start == start, "%s: %zu start nodes, expected %zu", what, out.start.size(), start.size());
    if (uniform) EXPECT(out.hub_rows.empty() && out.hub_off.empty(), "%s: hub rows on uniform weights", what);
    else EXPECT(out.hub_rows == hubs && out.hub_off == hoff, "%s: %zu hub rows, expected %zu", what, out.hub_rows.size(), hubs.size());
}

void check_refusal(const char *what, int64_t n, int64_t nnz, const int64_t *rp, const int32_t *col, const float *w, N2vGraphError::Kind kind, int64_t index)
{
    N2vGraph out;
    const N2vGraphError e = prepare_n2v_graph(n, nnz, rp, col, w, out);
    EXPECT(e.kind == kind && e.index == index, "%s: kind %d index %lld, expected %d at %lld", what, (int)e.kind, (long long)e.index, (int)kind, (long long)index);
}

int run_self()
{
    check_graph("unweighted, rows unsorted", random_csr(200, 30, false, false, 3), ALIAS_HUB_DEG);
    check_graph("weighted, rows unsorted", random_csr(200, 30, true, false, 3), ALIAS_HUB_DEG);
    check_graph("weights differ between rows only", random_csr(50, 12, true, true, 5), ALIAS_HUB_DEG);
    check_graph("hub rows at 8 neighbours", random_csr(60, 16, true, false, 7), 8);
    check_graph("sink and isolated ids", csr_of_edges(40, {0, 1, 2, 5, 5, 9, 30}, {1, 2, 0, 9, 2, 5, 31}), ALIAS_HUB_DEG);
    check_graph("one row repeats a column", Csr{3, {0, 4, 4, 5}, {2, 1, 2, 1, 0}, {1.f, 2.f, 3.f, 4.f, 5.f}}, ALIAS_HUB_DEG);
    using E = N2vGraphError;
    const int64_t rp[] = {0, 1, 3, 4}; const int32_t col[] = {1, 0, 2, 1}; const float w[] = {1.f, 2.f, 0.f, 1.f};
    check_refusal("n = 0", 0, 4, rp, col, nullptr, E::N_OUT_OF_RANGE, 0);
    check_refusal("n = 2^31 - 1", 0x7fffffff, 4, rp, col, nullptr, E::N_OUT_OF_RANGE, 0x7fffffff);
    check_refusal("no row_ptr", 3, 4, nullptr, col, nullptr, E::BAD_ARRAYS, -1);
    { const int64_t r[] = {1, 1, 3, 4}; check_refusal("row_ptr[0] = 1", 3, 4, r, col, nullptr, E::ROW_PTR_FIRST, 0); }
    { const int64_t r[] = {0, 1, 3, 3}; check_refusal("row_ptr[n] = 3", 3, 4, r, col, nullptr, E::ROW_PTR_LAST, 3); }
    { const int64_t r[] = {0, 3, 1, 4}; check_refusal("row_ptr falls", 3, 4, r, col, nullptr, E::ROW_PTR_NOT_MONOTONE, 1); }
    { const int32_t c[] = {1, 0, 3, -1}; check_refusal("column 3 of 3", 3, 4, rp, c, nullptr, E::COLUMN_OUT_OF_RANGE, 2); }
    check_refusal("weight 0", 3, 4, rp, col, w, E::NON_POSITIVE_WEIGHT, 2);

    // the renaming: 6 nodes, 4 of them occur in the order 4 0 5 2
    {
        const int32_t back[] = {4, 0, 5, 2}, K[] = {5, 0, 4, 0, 2, 0}; const float U[] = {0.5f, 0.f, 0.25f, 0.f, 1.f, 0.75f};
        float UT[4]; int32_t KT[4];
        unigram_table_renamed(6, 4, back, U, K, UT, KT);
        const float wantU[] = {1.f, 0.5f, 0.75f, 0.25f}; const int32_t wantK[] = {3, 2, 1, 0};
        EXPECT(!memcmp(UT, wantU, sizeof UT) && !memcmp(KT, wantK, sizeof KT), "renaming");
        unigram_table_renamed(6, 4, back, U, K, nullptr, nullptr);
    }
    // the knobs: nothing set, and every variable below / above its range
    EXPECT(knob_values(sgns_knobs_from_env(fake_lookup)) == knob_values(SgnsKnobs()), "knobs: empty environment");
    fake_env = {"GEMHIP_SGNS_MAX_WAVES=-5", "GEMHIP_SGNS_CACHE_R=99", "GEMHIP_SGNS_CACHE_DELTA=-9", "GEMHIP_SGNS_PREFETCH=0", "GEMHIP_SGNS_RELOAD=7", "GEMHIP_SGNS_HOT_COUNT=-3",
                "GEMHIP_SGNS_LOCAL_HOT=-1", "GEMHIP_SGNS_FRESH=13", "GEMHIP_SGNS_NEG_COUNT=junk"};
    EXPECT((knob_values(sgns_knobs_from_env(fake_lookup)) == std::vector<int>{0, 31, -1, 1, 1, -1, 0, 5, 0}), "knobs: clamps");
    fprintf(stderr, "n2v graph driver: %d failed checks\n", failures);
    return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "graph")) return run_graph(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "rename")) return run_rename(argv[2], argv[3]);
    if (argc >= 2 && !strcmp(argv[1], "knobs")) return run_knobs(argc - 2, argv + 2);
    if (argc == 2 && !strcmp(argv[1], "self")) return run_self();
    fprintf(stderr, "usage: %s graph <in> <out> | rename <in> <out> | knobs [NAME=VALUE ...] | self\n", argv[0]);
    return 2;
}
