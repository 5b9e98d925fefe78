// n2v_graph.hpp -- the host arithmetic of node2vec's graph set-up (n2v_graph.hip): what gemhip_n2v_create derives from a CSR before its first HIP
// call, and the renaming of the binary-layout unigram table.  Plain C++, no HIP: everything here runs on a CPU (scripts/build_asan_n2v_graph.sh,
// tests/test_n2v_graph.py); n2v.hip words the refusals, allocates and uploads.
#pragma once
#include <cstdint>
#include <vector>

namespace gemhip {

constexpr int ALIAS_HUB_DEG = 2048;      // rows from this many neighbours on take n2v_alias_hub_kernel (oracle: ORACLE_ALIAS_HUB_DEG)

// What prepare_n2v_graph found wrong with a CSR.  It never words a message: gemhip_n2v_create does.
struct N2vGraphError {
    enum Kind { NONE = 0, N_OUT_OF_RANGE, BAD_ARRAYS, ROW_PTR_FIRST, ROW_PTR_LAST, ROW_PTR_NOT_MONOTONE, COLUMN_OUT_OF_RANGE, NON_POSITIVE_WEIGHT } kind = NONE;
    int64_t index = -1;                // the first offender: entry of row_ptr (ROW_PTR_FIRST: 0, ROW_PTR_LAST: n), row (ROW_PTR_NOT_MONOTONE), edge (the last two)
    int32_t column = 0;                // COLUMN_OUT_OF_RANGE: the column found there
    explicit operator bool() const { return kind != NONE; }
};

struct N2vGraph {
    std::vector<int32_t> col;          // columns sorted inside each row (the has_edge test of the 2nd-order walk bisects them)
    std::vector<float> w;              // the weights that followed them (stable sort: equal columns keep their order); empty without weights
    bool uniform = true;               // every row has equal weights -> no alias tables needed
    std::vector<int32_t> start;        // walk start nodes, ascending: the nodes that occur in the edge list (an isolated node never starts a walk)
    std::vector<int32_t> hub_rows;     // weighted graphs: rows with at least hub_deg neighbours (n2v_alias_hub_kernel builds their tables) ...
    std::vector<int64_t> hub_off;      // ... and the offset of each one's scratch segment (prefix sum of their degrees; hub_rows.size() + 1 entries)
};

// Validates the CSR (the checks in the order gemhip_n2v_create has always made them: the first failure is the one reported) and fills `out`.
// w may be null (unit weights).  On an error `out` is unspecified.
N2vGraphError prepare_n2v_graph(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, N2vGraph &out, int hub_deg = ALIAS_HUB_DEG);

// gemhip_n2v_build_unigram_vocab_order's UT_out / KT_out.  The builder stores the table by node (U, K over n nodes); entry r of the binary's table is
// node back[r] (back: the n_vocab nodes that occur, in first-appearance order), its alias the renamed id of that node's alias.  Either output may be null.
void unigram_table_renamed(int64_t n, int64_t n_vocab, const int32_t *back, const float *U, const int32_t *K, float *UT_out, int32_t *KT_out);

}  // namespace gemhip
