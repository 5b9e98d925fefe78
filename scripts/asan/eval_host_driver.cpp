// Stand-alone driver of gem_amd/csrc/eval_host.hip (the evaluator's host arithmetic: CSR check, mask normal form, AP chunks, AP from counts): plain
// C++, no HIP, no device.  Every form reads one binary file and writes one; integers are int64 unless named otherwise.
//
//   eval_host_driver check <in> <out>
//       in:  n, len_col (-1: a null col), row_ptr[n + 1], int32 col[len_col]           out: kind, index, column, sorted
//   eval_host_driver mask <in> <out>
//       in:  n, len_col, row_ptr[n + 1], int32 col[len_col]                             out: row_ptr[n + 1], int32 col[row_ptr[n]]
//   eval_host_driver chunks <in> <out>
//       in:  n, len_col, len_mask_col (-1: no mask), undirected, nsample, row_ptr[n + 1], int32 col[len_col],
//            and with a mask: mask_row_ptr[n + 1], int32 mask_col[len_mask_col] (as `mask` wrote them); int32 nodes[nsample]
//       out: total, nchunk, node_off[nsample + 1], chunk_off[nchunk], int32 nb[total], int32 chunk_node[nchunk], int32 chunk_cnt[nchunk]
//   eval_host_driver ap <in> <out>
//       in:  nsample, total, want_npos, node_off[nsample + 1], double score[total], int32 nb[total], int32 count[total]
//       out: double ap[nsample], npos[nsample] (filled with -7 when want_npos is 0: ap_from_counts is then given a null pointer)
//
// tests/test_eval_host.py drives all four; scripts/build_asan_eval.sh runs the same tests through a build with AddressSanitizer and UBSan.
#include "../../gem_amd/csrc/eval_host.hpp"
#include <cstdio>
#include <cstring>

using namespace gemhip;

namespace {

template <typename T> bool read_vec(FILE *f, std::vector<T> &v, int64_t count)
{
    v.resize((size_t)(count > 0 ? count : 0));
    return count <= 0 || fread(v.data(), sizeof(T), (size_t)count, f) == (size_t)count;
}
template <typename T> void write_vec(FILE *f, const std::vector<T> &v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

struct Csr {
    int64_t n = 0, len_col = 0; std::vector<int64_t> rp; std::vector<int32_t> col;
    bool read(FILE *f) { return read_vec(f, rp, n + 1) && read_vec(f, col, len_col); }
    const int32_t *cols() const { return len_col < 0 ? nullptr : col.data(); }
};

int run(const char *mode, FILE *f, FILE *o)
{
    if (!strcmp(mode, "check") || !strcmp(mode, "mask")) {
        Csr g;
        if (fread(&g.n, 8, 1, f) != 1 || fread(&g.len_col, 8, 1, f) != 1 || !g.read(f)) return 2;
        if (!strcmp(mode, "check")) {
            bool sorted = true;
            const EvalCsrError e = check_eval_csr(g.n, g.rp.data(), g.cols(), &sorted);
            const int64_t out[4] = {(int64_t)e.kind, e.index, (int64_t)e.column, e ? -1 : (int64_t)sorted};
            fwrite(out, 8, 4, o);
        } else {
            const EvalMask m = normalise_mask(g.n, g.rp.data(), g.cols());
            write_vec(o, m.row_ptr); write_vec(o, m.col);
        }
        return 0;
    }
    if (!strcmp(mode, "chunks")) {
        int64_t hdr[5];
        Csr g, m; std::vector<int32_t> nodes;
        if (fread(hdr, 8, 5, f) != 5) return 2;
        g.n = m.n = hdr[0]; g.len_col = hdr[1]; m.len_col = hdr[2];
        if (!g.read(f) || (hdr[2] >= 0 && !m.read(f)) || !read_vec(f, nodes, hdr[4])) return 2;
        const ApChunks c = ap_chunks(g.rp.data(), g.col.data(), hdr[2] >= 0 ? m.rp.data() : nullptr, hdr[2] >= 0 ? m.col.data() : nullptr, hdr[3] != 0, hdr[4], nodes.data());
        const int64_t sizes[2] = {(int64_t)c.nb.size(), (int64_t)c.chunk_node.size()};
        fwrite(sizes, 8, 2, o);
        write_vec(o, c.node_off); write_vec(o, c.chunk_off); write_vec(o, c.nb); write_vec(o, c.chunk_node); write_vec(o, c.chunk_cnt);
        return 0;
    }
    if (!strcmp(mode, "ap")) {
        int64_t hdr[3];
        std::vector<int64_t> node_off; std::vector<double> score; std::vector<int32_t> nb, count;
        if (fread(hdr, 8, 3, f) != 3 || !read_vec(f, node_off, hdr[0] + 1) || !read_vec(f, score, hdr[1]) || !read_vec(f, nb, hdr[1]) || !read_vec(f, count, hdr[1])) return 2;
        std::vector<double> ap((size_t)hdr[0], -1.0); std::vector<int64_t> npos((size_t)hdr[0], -7);
        ap_from_counts(hdr[0], nb.data(), node_off.data(), score.data(), count.data(), ap.data(), hdr[2] ? npos.data() : nullptr);
        write_vec(o, ap); write_vec(o, npos);
        return 0;
    }
    return 2;
}

}  // namespace

int main(int argc, char **argv)
{
    FILE *f = argc == 4 ? fopen(argv[2], "rb") : nullptr, *o = argc == 4 ? fopen(argv[3], "wb") : nullptr;
    int rc = f && o ? run(argv[1], f, o) : 2;
    if (f) fclose(f);
    if (o && fclose(o)) rc = 2;
    if (rc) fprintf(stderr, "usage: %s check|mask|chunks|ap <in> <out>  (or a malformed <in>)\n", argv[0]);
    return rc;
}
