// n2v_graph.hip -- the host arithmetic of node2vec's graph set-up: CSR validation, the per-row stable sort with weights following, the
// uniform-weights flag, the walk start nodes, the hub rows of the alias build; and the renaming of the binary-layout unigram table.
// HIP-free by rule: no HIP header, nothing from common.hpp -- the `.hip` suffix only serves the build's csrc/*.hip glob, and the file is also valid
// `clang++ -x c++ -std=c++17` input (scripts/build_asan_n2v_graph.sh runs it under AddressSanitizer / UBSan, tests/test_n2v_graph.py compares it with
// the oracle's sorted CSR and start nodes).  n2v.hip holds the C ABI around it.
#include "n2v_graph.hpp"
#include <algorithm>
#include <utility>

namespace gemhip {

N2vGraphError prepare_n2v_graph(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, N2vGraph &out, int hub_deg)
{
    using E = N2vGraphError;
    if (!(n > 0 && n < (int64_t)0x7fffffff)) return E{E::N_OUT_OF_RANGE, n};
    if (!(nnz >= 0 && row_ptr && (nnz == 0 || col))) return E{E::BAD_ARRAYS};
    if (row_ptr[0] != 0) return E{E::ROW_PTR_FIRST, 0};
    if (row_ptr[n] != nnz) return E{E::ROW_PTR_LAST, n};
    // sort columns inside each row (needed by the has_edge test of the 2nd-order walk); weights follow
    std::vector<int32_t> &c = out.col;
    std::vector<float> &ww = out.w;
    c.assign(col, col + nnz);
    ww.clear();
    if (w) ww.assign(w, w + nnz);
    bool uniform = true;
    std::vector<std::pair<int32_t, float>> tmp;
    for (int64_t v = 0; v < n; ++v) {
        const int64_t a = row_ptr[v], b = row_ptr[v + 1];
        if (!(a <= b && b <= nnz)) return E{E::ROW_PTR_NOT_MONOTONE, v};
        bool sorted = true;
        for (int64_t e = a; e < b; ++e) {
            if (!(c[e] >= 0 && c[e] < n)) return E{E::COLUMN_OUT_OF_RANGE, e, c[e]};
            if (e > a && c[e] < c[e - 1]) sorted = false;
            if (w && w[e] != w[a]) uniform = false;
            if (w && !(w[e] > 0.f)) return E{E::NON_POSITIVE_WEIGHT, e};
        }
        if (!sorted) {
            tmp.clear();
            for (int64_t e = a; e < b; ++e) tmp.emplace_back(c[e], w ? ww[e] : 1.f);
            std::stable_sort(tmp.begin(), tmp.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
            for (int64_t e = a; e < b; ++e) { c[e] = tmp[e - a].first; if (w) ww[e] = tmp[e - a].second; }
        }
    }
    out.uniform = uniform;
    out.start.clear();
    {
        std::vector<char> present(n, 0);
        for (int64_t v = 0; v < n; ++v)
            if (row_ptr[v + 1] > row_ptr[v]) present[v] = 1;
        for (int64_t e = 0; e < nnz; ++e) present[c[e]] = 1;
        for (int64_t v = 0; v < n; ++v) if (present[v]) out.start.push_back((int32_t)v);
    }
    out.hub_rows.clear(); out.hub_off.clear();
    if (!uniform) {
        out.hub_off.push_back(0);
        for (int64_t v = 0; v < n; ++v)
            if (row_ptr[v + 1] - row_ptr[v] >= hub_deg) { out.hub_rows.push_back((int32_t)v); out.hub_off.push_back(out.hub_off.back() + (row_ptr[v + 1] - row_ptr[v])); }
    }
    return E{};
}

void unigram_table_renamed(int64_t n, int64_t n_vocab, const int32_t *back, const float *U, const int32_t *K, float *UT_out, int32_t *KT_out)
{
    if (UT_out) for (int64_t r = 0; r < n_vocab; ++r) UT_out[r] = U[back[r]];
    if (KT_out) {
        std::vector<int32_t> renamed(n, 0);
        for (int64_t r = 0; r < n_vocab; ++r) renamed[back[r]] = (int32_t)r;
        for (int64_t r = 0; r < n_vocab; ++r) KT_out[r] = renamed[K[back[r]]];
    }
}

}  // namespace gemhip
