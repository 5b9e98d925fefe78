// Stand-alone AddressSanitizer driver for the HOST part of the evaluator handle (gem_amd/csrc/eval.hip: gemhip_eval_create's validation and host copies,
// the NULL-handle refusals of gemhip_eval_ap / gemhip_eval_pairs, gemhip_eval_destroy).  Built and run by scripts/build_asan_eval.sh on a machine WITHOUT
// a GPU: a well-formed create then gets as far as its first HIP call, fails with GEMHIP_E_HIP and must release everything it copied.  With a GPU the same
// program goes on to score a few pairs on the host-validated path.
#include "../../include/gem_hip.h"
#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s  [last error: %s]\n", __LINE__, #cond, gemhip_last_error()); ++failures; } } while (0)

int main()
{
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
