// Stand-alone AddressSanitizer driver for the HOST part of the evaluator handle (gem_amd/csrc/eval.hip: gemhip_eval_create's validation and host copies,
// the NULL-handle refusals of gemhip_eval_ap / gemhip_eval_pairs, gemhip_eval_destroy).  Built and run by scripts/build_asan_eval.sh on a machine WITHOUT
// a GPU: a well-formed create then gets as far as its first HIP call, fails with GEMHIP_E_HIP and must release everything it copied.  With a GPU the same
// program goes on to score a few pairs on the host-validated path.  Before that it calls the four device-free functions of gem_amd/csrc/eval_host.hip
// directly, on the shapes of tests/test_eval_host.py in C++: a 700-node graph with a hub of 600 neighbours (two chunks), rows of 512 and 513, an empty
// row, a row of lower ids only, an unsorted row with a repeated column, a mask with unsorted rows and repeats, and repeated sample nodes.
#include "../../include/gem_hip.h"
#include "../../gem_amd/csrc/eval_host.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s  [last error: %s]\n", __LINE__, #cond, gemhip_last_error()); ++failures; } } while (0)

// ---- the host half, called directly
static void host_half()
{
    using namespace gemhip;
    const int64_t n = 700;
    std::vector<std::vector<int32_t>> rows(n), mrows(n);
    for (int32_t t = 0; t < 600; ++t) rows[2].push_back(699 - t);                      // the hub, descending
    for (int32_t t = 0; t < 512; ++t) rows[5].push_back(6 + t);
    for (int32_t t = 0; t < 513; ++t) rows[9].push_back(10 + t);
    rows[650] = {4, 17, 649}; rows[20] = {400, 17, 400, 333, 21, 20};                   // lower ids only; unsorted, 400 twice, a self-loop; row 11 stays empty
    for (int32_t i = 30; i < 600; i += 7) rows[i] = {i + 3, i - 2, i + 90};
    mrows[5].assign(rows[5].begin(), rows[5].begin() + 400); mrows[20] = {500, 17, 500, 77}; mrows[9] = {3, 2, 1}; mrows[11] = {3, 50, 600};
    auto csr = [&](const std::vector<std::vector<int32_t>> &r, std::vector<int64_t> &rp, std::vector<int32_t> &col) {
        rp.assign(1, 0); col.clear();
        for (const auto &x : r) { col.insert(col.end(), x.begin(), x.end()); rp.push_back((int64_t)col.size()); }
    };
    std::vector<int64_t> rp, mrp; std::vector<int32_t> col, mcol;
    csr(rows, rp, col); csr(mrows, mrp, mcol);
    bool sorted = true;
    EXPECT(!check_eval_csr(n, rp.data(), col.data(), &sorted) && !sorted);
    EXPECT(!check_eval_csr(n, mrp.data(), mcol.data(), nullptr));
    { auto bad = col; bad.back() = 700; const EvalCsrError e = check_eval_csr(n, rp.data(), bad.data(), &sorted);
      EXPECT(e.kind == EvalCsrError::COLUMN_OUT_OF_RANGE && e.index == (int64_t)col.size() - 1 && e.column == 700); }
    { auto bad = rp; bad[3] = bad[2] - 1; const EvalCsrError e = check_eval_csr(n, bad.data(), col.data(), &sorted); EXPECT(e.kind == EvalCsrError::ROW_PTR_DECREASES && e.index == 2); }
    { auto bad = rp; bad[0] = 1; EXPECT(check_eval_csr(n, bad.data(), col.data(), nullptr).kind == EvalCsrError::ROW_PTR_FIRST); }
    EXPECT(check_eval_csr(n, rp.data(), nullptr, nullptr).kind == EvalCsrError::COL_NULL);
    const EvalMask m = normalise_mask(n, mrp.data(), mcol.data());
    for (int64_t i = 0; i < n; ++i) {
        const std::set<int32_t> want(mrows[i].begin(), mrows[i].end());
        EXPECT(std::vector<int32_t>(m.col.begin() + m.row_ptr[i], m.col.begin() + m.row_ptr[i + 1]) == std::vector<int32_t>(want.begin(), want.end()));
    }
    std::vector<int32_t> nodes;
    for (int32_t i = 0; i < n; ++i) nodes.push_back(i);
    for (int32_t i : {2, 2, 9, 11}) nodes.push_back(i);                                 // repeats: slices of their own
    for (int masked = 0; masked < 2; ++masked)
        for (int und = 0; und < 2; ++und) {
            const ApChunks c = ap_chunks(rp.data(), col.data(), masked ? m.row_ptr.data() : nullptr, masked ? m.col.data() : nullptr, und != 0, (int64_t)nodes.size(), nodes.data());
            size_t chunk = 0;
            for (size_t k = 0; k < nodes.size(); ++k) {
                const int32_t i = nodes[k];
                std::set<int32_t> want;
                for (int32_t t : rows[i]) if (t != i && !(und && t < i) && !(masked && std::count(mrows[i].begin(), mrows[i].end(), t))) want.insert(t);
                EXPECT(c.node_off[k + 1] - c.node_off[k] == (int64_t)want.size());
                EXPECT(std::equal(want.begin(), want.end(), c.nb.begin() + c.node_off[k]));
                for (size_t o = 0; o < want.size(); o += EV_MAXNB, ++chunk)
                    EXPECT(chunk < c.chunk_node.size() && c.chunk_node[chunk] == i && c.chunk_off[chunk] == c.node_off[k] + (int64_t)o &&
                           c.chunk_cnt[chunk] == (int32_t)std::min<size_t>(EV_MAXNB, want.size() - o));
            }
            EXPECT(chunk == c.chunk_node.size() && c.node_off.back() == (int64_t)c.nb.size());
            // scores with ties (a third of the ids share a value) and some not positive; counts as the kernel streams them, restated per neighbour
            auto score_of = [](int32_t i, int32_t j) { return (double)((i * 7 + j / 3) % 11) - 2.0; };
            std::vector<double> sc(c.nb.size()); std::vector<int32_t> cnt(c.nb.size());
            for (size_t k = 0; k < nodes.size(); ++k)
                for (int64_t e = c.node_off[k]; e < c.node_off[k + 1]; ++e) {
                    const int32_t i = nodes[k], t = c.nb[e];
                    sc[e] = score_of(i, t); cnt[e] = 0;
                    for (int32_t j = und ? i + 1 : 0; j < n; ++j) {
                        if (j == i || (masked && std::binary_search(m.col.begin() + m.row_ptr[i], m.col.begin() + m.row_ptr[i + 1], j)) || !(score_of(i, j) > 0.0)) continue;
                        cnt[e] += score_of(i, j) > sc[e] || (score_of(i, j) == sc[e] && j < t);
                    }
                }
            std::vector<double> ap(nodes.size(), -1.0); std::vector<int64_t> npos(nodes.size(), -1);
            ap_from_counts((int64_t)nodes.size(), c.nb.data(), c.node_off.data(), sc.data(), cnt.data(), ap.data(), npos.data());
            for (size_t k = 0; k < nodes.size(); ++k) {                                 // AP from the full ranking of node k's candidates
                const int32_t i = nodes[k];
                std::vector<std::pair<double, int32_t>> cand;                           // (-score, id): ascending = the evaluator's order
                for (int32_t j = und ? i + 1 : 0; j < n; ++j)
                    if (j != i && !(masked && std::binary_search(m.col.begin() + m.row_ptr[i], m.col.begin() + m.row_ptr[i + 1], j)) && score_of(i, j) > 0.0) cand.emplace_back(-score_of(i, j), j);
                std::sort(cand.begin(), cand.end());
                double sum = 0.0; int64_t hits = 0;
                for (size_t r = 0; r < cand.size(); ++r)
                    if (std::binary_search(c.nb.begin() + c.node_off[k], c.nb.begin() + c.node_off[k + 1], cand[r].second)) { ++hits; sum += (double)hits / (double)(r + 1); }
                EXPECT(npos[k] == hits && ap[k] == (hits ? sum / (double)hits : 0.0));
            }
            ap_from_counts((int64_t)nodes.size(), c.nb.data(), c.node_off.data(), sc.data(), cnt.data(), ap.data(), nullptr);
        }
    std::printf("host half: check_eval_csr, normalise_mask, ap_chunks and ap_from_counts on the 700-node shapes\n");
}

int main()
{
    host_half();
    const int64_t n = 5; const int32_t d = 3, ld = 4;
    std::vector<float> X((size_t)n * ld, 0.5f);
    std::vector<int64_t> rp = {0, 2, 2, 3, 5, 5};
    std::vector<int32_t> col = {1, 4, 0, 0, 2};
    gemhip_eval_t h = (gemhip_eval_t)0x1;
    EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 2, rp.data(), col.data(), &h) == GEMHIP_E_INVALID && h == nullptr);
    EXPECT(std::strstr(gemhip_last_error(), "kind 2") != nullptr);
    EXPECT(gemhip_eval_create(n, d, ld, X.data(), X.data() + 1, 1, rp.data(), col.data(), &h) == GEMHIP_E_INVALID);      // kind 1 with a second operand
    EXPECT(gemhip_eval_create(n, 513, 513, X.data(), nullptr, 0, rp.data(), col.data(), &h) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_create(n, d, 2, X.data(), nullptr, 0, rp.data(), col.data(), &h) == GEMHIP_E_INVALID);           // ld < da
    EXPECT(gemhip_eval_create(n, d, ld, nullptr, nullptr, 0, rp.data(), col.data(), &h) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, rp.data(), col.data(), nullptr) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, rp.data(), nullptr, &h) == GEMHIP_E_INVALID);             // nnz > 0 without columns
    { auto bad = rp; bad[0] = 1; EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, bad.data(), col.data(), &h) == GEMHIP_E_INVALID); }
    { auto bad = rp; bad[2] = 1; EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, bad.data(), col.data(), &h) == GEMHIP_E_INVALID);
      EXPECT(std::strstr(gemhip_last_error(), "row_ptr decreases at row 1") != nullptr); }
    { auto bad = col; bad[4] = 5; EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, rp.data(), bad.data(), &h) == GEMHIP_E_INVALID);
      EXPECT(std::strstr(gemhip_last_error(), "column 5 outside [0,5)") != nullptr); }
    { auto bad = col; bad[0] = -1; EXPECT(gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, rp.data(), bad.data(), &h) == GEMHIP_E_INVALID); }
    double s[4]; uint8_t hit[4]; int32_t st[4] = {0, 3, 2, 4}, ed[4] = {4, 2, 2, 0};
    EXPECT(gemhip_eval_pairs(nullptr, 4, st, ed, s, hit) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_ap(nullptr, 1, 4, st, s) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_last_pairs_ms(nullptr, s) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_set_mask(nullptr, rp.data(), col.data()) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_ap_masked(nullptr, 1, 4, st, s, nullptr) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_topk(nullptr, 1, 1, 4, st, 1, ed, s, hit) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_last_kernel_ms(nullptr, s) == GEMHIP_E_INVALID);
    EXPECT(gemhip_eval_destroy(nullptr) == GEMHIP_OK);
    const int rc = gemhip_eval_create(n, d, ld, X.data(), nullptr, 0, rp.data(), col.data(), &h);     // well-formed
    if (rc == GEMHIP_OK) {
        EXPECT(h != nullptr);
        EXPECT(gemhip_eval_pairs(h, 0, nullptr, nullptr, nullptr, nullptr) == GEMHIP_OK);
        int32_t bad_st[4] = {0, 3, 5, 4};
        EXPECT(gemhip_eval_pairs(h, 4, bad_st, ed, s, hit) == GEMHIP_E_INVALID);
        EXPECT(gemhip_eval_pairs(h, 4, st, bad_st, s, nullptr) == GEMHIP_E_INVALID);
        EXPECT(gemhip_eval_pairs(h, 4, st, ed, s, hit) == GEMHIP_OK);
        EXPECT(hit[0] == 1 && hit[1] == 1 && hit[2] == 0 && hit[3] == 0 && s[2] == 0.0 && s[0] == 0.75);
        // link prediction: the mask is validated, copied, sorted and de-duplicated on the host
        std::vector<int64_t> mrp = {0, 3, 3, 3, 4, 4}; std::vector<int32_t> mcol = {4, 2, 4, 0};
        { auto bad = mcol; bad[1] = 5; EXPECT(gemhip_eval_set_mask(h, mrp.data(), bad.data()) == GEMHIP_E_INVALID); }
        { auto bad = mrp; bad[2] = 2; EXPECT(gemhip_eval_set_mask(h, bad.data(), mcol.data()) == GEMHIP_E_INVALID); }
        EXPECT(gemhip_eval_set_mask(h, mrp.data(), mcol.data()) == GEMHIP_OK);
        int32_t nodes[2] = {0, 3}, ids[4]; double ap[2], sc[4]; int64_t npos[2]; uint8_t th[4];
        EXPECT(gemhip_eval_ap_masked(h, 0, 2, nodes, ap, npos) == GEMHIP_OK && npos[0] == 1 && npos[1] == 1);     // 0 -> 4 and 3 -> 0 are masked
        EXPECT(gemhip_eval_topk(h, 0, 1, 2, nodes, 0, ids, sc, th) == GEMHIP_E_INVALID);
        EXPECT(gemhip_eval_topk(h, 0, 1, 2, nodes, 2, ids, sc, th) == GEMHIP_OK && ids[0] == 1 && ids[1] == 3 && th[0] == 1 && th[1] == 0);
        EXPECT(gemhip_eval_set_mask(h, nullptr, nullptr) == GEMHIP_OK);
        EXPECT(gemhip_eval_destroy(h) == GEMHIP_OK);
        std::printf("device present: scored 4 pairs, masked AP and top-2 of 2 nodes\n");
    } else {
        EXPECT(rc == GEMHIP_E_HIP && h == nullptr);
        std::printf("no device: a well-formed create stopped at its first HIP call (%s)\n", gemhip_last_error());
    }
    std::printf("eval driver: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
