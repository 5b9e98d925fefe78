// eval_host.hpp -- the host arithmetic of the evaluator handle (eval_host.hip): the CSR check of gemhip_eval_create / gemhip_eval_set_mask, the
// mask's normal form, and the two halves of an AP call around its kernel -- the candidate chunks before, AP from (score, count) after.
// Plain C++, no HIP: everything here runs on a CPU (scripts/build_asan_eval.sh, tests/test_eval_host.py); eval.hip words the refusals, uploads
// and launches.
#pragma once
#include <cstdint>
#include <vector>

namespace gemhip {

constexpr int EV_MAXNB = 512;          // true neighbours per chunk: eval_ap_kernel holds a chunk in registers, ap_chunks cuts the rows to it

// What check_eval_csr found wrong with a CSR.  It never words a message: gemhip_eval_create and gemhip_eval_set_mask do.
struct EvalCsrError {
    enum Kind { NONE = 0, ROW_PTR_FIRST, ROW_PTR_DECREASES, COL_NULL, COLUMN_OUT_OF_RANGE } kind = NONE;
    int64_t index = -1;                // the first offender: entry 0 of row_ptr (ROW_PTR_FIRST), the row (ROW_PTR_DECREASES), the edge (COLUMN_OUT_OF_RANGE)
    int32_t column = 0;                // COLUMN_OUT_OF_RANGE: the column found there
    explicit operator bool() const { return kind != NONE; }
};

// The checks in the order the evaluator has always made them (the first failure is the one reported): row_ptr[0] == 0, no row of negative
// length, columns present when there are edges, every column in [0, n).  row_ptr has n + 1 entries, n >= 1.  *sorted (may be null): no row
// lists a column below its predecessor -- equal neighbours count as sorted.  On an error *sorted is unspecified.
EvalCsrError check_eval_csr(int64_t n, const int64_t *row_ptr, const int32_t *col, bool *sorted);

// A checked CSR in the form the kernels' mask cursor walks: every row ascending, each column once.
struct EvalMask { std::vector<int64_t> row_ptr; std::vector<int32_t> col; };
EvalMask normalise_mask(int64_t n, const int64_t *row_ptr, const int32_t *col);

// The positives of every sampled node, cut into the kernel's workgroups.  Node nodes[k] owns nb[node_off[k] .. node_off[k + 1]): its true
// neighbours t != i (t > i when undirected) that are not mask arcs, ascending, each once.  Chunk c is chunk_cnt[c] <= EV_MAXNB of them from
// nb[chunk_off[c]] on, for node chunk_node[c]; a node without positives has no chunk.  A node sampled twice gets two slices.
struct ApChunks { std::vector<int32_t> nb, chunk_node, chunk_cnt; std::vector<int64_t> chunk_off, node_off; };
// row_ptr / col: the checked CSR (rows in any order, repeats allowed); mask_row_ptr / mask_col: a normalise_mask result, or both null.
ApChunks ap_chunks(const int64_t *row_ptr, const int32_t *col, const int64_t *mask_row_ptr, const int32_t *mask_col, bool undirected, int64_t nsample,
                   const int32_t *nodes);

// AP_i = mean over the positives with score > 0 of rank_hit / rank_all: rank_hit = the place among those positives in the evaluator's order
// (score descending, node id ascending on ties), rank_all = 1 + count (the kernel's streamed count of candidates that rank before).  score
// and count run parallel to nb.  ap_out[k] = 0 without such a positive; npos_out (may be null) is their number.
void ap_from_counts(int64_t nsample, const int32_t *nb, const int64_t *node_off, const double *score, const int32_t *count, double *ap_out, int64_t *npos_out);

}  // namespace gemhip
