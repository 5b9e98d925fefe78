// eval_host.hip -- the evaluator's host arithmetic (eval_host.hpp).  No HIP header, no device code: builds with a plain C++ compiler.
#include "eval_host.hpp"
#include <algorithm>

namespace gemhip {

EvalCsrError check_eval_csr(int64_t n, const int64_t *row_ptr, const int32_t *col, bool *sorted)
{
    EvalCsrError err;
    if (row_ptr[0] != 0) { err.kind = EvalCsrError::ROW_PTR_FIRST; err.index = 0; return err; }
    for (int64_t i = 0; i < n; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) { err.kind = EvalCsrError::ROW_PTR_DECREASES; err.index = i; return err; }
    if (row_ptr[n] != 0 && !col) { err.kind = EvalCsrError::COL_NULL; return err; }
    bool asc = true;
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) { err.kind = EvalCsrError::COLUMN_OUT_OF_RANGE; err.index = e; err.column = col[e]; return err; }
            if (e > row_ptr[i] && col[e] < col[e - 1]) asc = false;
        }
    if (sorted) *sorted = asc;
    return err;
}

EvalMask normalise_mask(int64_t n, const int64_t *row_ptr, const int32_t *col)
{
    EvalMask m;
    m.row_ptr.assign(n + 1, 0); m.col.reserve(row_ptr[n]);
    for (int64_t i = 0; i < n; ++i) {
        const size_t first = m.col.size();
        m.col.insert(m.col.end(), col + row_ptr[i], col + row_ptr[i + 1]);
        std::sort(m.col.begin() + first, m.col.end());
        m.col.erase(std::unique(m.col.begin() + first, m.col.end()), m.col.end());
        m.row_ptr[i + 1] = (int64_t)m.col.size();
    }
    return m;
}

ApChunks ap_chunks(const int64_t *row_ptr, const int32_t *col, const int64_t *mask_row_ptr, const int32_t *mask_col, bool undirected, int64_t nsample,
                   const int32_t *nodes)
{
    ApChunks c;
    c.node_off.assign(nsample + 1, 0);
    std::vector<int32_t> tmp;
    for (int64_t k = 0; k < nsample; ++k) {
        const int i = nodes[k];
        tmp.clear();
        const int32_t *mb = mask_row_ptr ? mask_col + mask_row_ptr[i] : nullptr, *me = mask_row_ptr ? mask_col + mask_row_ptr[i + 1] : nullptr;
        for (int64_t e = row_ptr[i]; e < row_ptr[i + 1]; ++e) {
            const int t = col[e];
            if (t == i || (undirected && t < i)) continue;
            if (mask_row_ptr && std::binary_search(mb, me, t)) continue;
            tmp.push_back(t);
        }
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        for (size_t o = 0; o < tmp.size(); o += EV_MAXNB) {
            c.chunk_node.push_back(i); c.chunk_off.push_back((int64_t)c.nb.size() + (int64_t)o);
            c.chunk_cnt.push_back((int32_t)std::min<size_t>(EV_MAXNB, tmp.size() - o));
        }
        c.nb.insert(c.nb.end(), tmp.begin(), tmp.end());
        c.node_off[k + 1] = (int64_t)c.nb.size();
    }
    return c;
}

void ap_from_counts(int64_t nsample, const int32_t *nb, const int64_t *node_off, const double *score, const int32_t *count, double *ap_out, int64_t *npos_out)
{
    std::vector<int64_t> ord;
    for (int64_t k = 0; k < nsample; ++k) {
        ord.clear();
        for (int64_t e = node_off[k]; e < node_off[k + 1]; ++e) if (score[e] > 0.0) ord.push_back(e);
        std::sort(ord.begin(), ord.end(), [&](int64_t x, int64_t y) { return score[x] > score[y] || (score[x] == score[y] && nb[x] < nb[y]); });
        double sum = 0.0;
        for (size_t r = 0; r < ord.size(); ++r) sum += (double)(r + 1) / (double)(1 + count[ord[r]]);
        ap_out[k] = ord.empty() ? 0.0 : sum / (double)ord.size();
        if (npos_out) npos_out[k] = (int64_t)ord.size();
    }
}

}  // namespace gemhip
