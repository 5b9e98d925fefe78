// eval.hip -- graph-reconstruction average precision of sampled nodes on the GPU.
//
// Reference: evaluateStaticGraphReconstruction (gem/evaluation/evaluate_graph_reconstruction.py:8-46) builds
// the n x n matrix of get_edge_weight(i, j) with an O(n^2) Python loop (static_graph_embedding.py:60-64), lists
// the pairs i<j with weight > 0 (gem/utils/evaluation_util.py:28-35), sorts every node's candidates by weight
// (stable, descending) and averages precision at the true edges (gem/evaluation/metrics.py:6-46).  That is
// unusable beyond n ~ 1e4, yet MAP is the parity metric of this backend at 1M nodes.
//
// AP of node i does not need a sort: for every true neighbour t,
//     rank_all(t) = 1 + #{candidates j : s_j > s_t  or (s_j == s_t and j < t)}      (stable tie rule)
//     rank_hit(t) = the same count restricted to true neighbours
//     AP_i = (1/H) sum_t rank_hit(t) / rank_all(t)       over the H neighbours with s_t > 0.
// One workgroup per (sampled node, chunk of <= 512 of its true neighbours) streams all rows B_j once (a wavefront per row,
// lanes across the d columns, fp64 dot of the fp32 inputs so ranks agree with the float64 reference), and every lane
// compares the score of the row with "its" neighbours' scores -- O(n d) per chunk, exact, no n x n matrix.  The kernel
// returns (score, rank_all - 1) per true neighbour; rank_hit is a sort of <= deg(i) numbers, done on the host.
// score(i, j) = A_i . B_j : A = B = X for GF / node2vec (X_i . X_j), A = X[:, :k], B = X[:, k:] for HOPE (hope.py:43-44).
// kind 1 (Laplacian Eigenmaps, LLE): score(i, j) = exp(-(sqrt(sum_k (x_ik - x_jk)^2))^2), the scalar get_edge_weight of lap.py:74 / lle.py:53 in fp64
// (differences of the fp32 inputs are exact in fp64; sqrt, then square, then exp).  Ranks and ties are decided on the exp OUTPUT: where exp saturates,
// distinct distances fall into one tie class and the node id decides, as in the reference -- the classes are those of the device's fp64 exp.
//
// The evaluator handle (gemhip_eval_create) keeps the embedding and the CSR of the true graph on the device for three consumers:
//   gemhip_eval_ap     the AP kernel above for sampled nodes;
//   gemhip_eval_pairs  score + "is (st -> ed) an edge" for an explicit pair list: the reference's pair-sampled MAP / precision curve
//                      (evaluation_util.py:5-26) and, over the edge list, its weighted reconstruction error (evaluate_graph_reconstruction.py:38-42).
// and, with a second graph as a mask (gemhip_eval_set_mask: the TRAIN graph of a link-prediction split, the handle's CSR being the TEST graph):
//   gemhip_eval_ap_masked  the same AP with the training arcs taken out of every candidate list;
//   gemhip_eval_topk       every sampled node's k best candidates, in the evaluator's order.
// This file holds the kernels, the handle and the entry points; what the host computes around the launches (the CSR check, the mask's normal form,
// the chunks, AP from the counts) is eval_host.hip, which needs no device.
#include "eval_common.hpp"
#include "eval_host.hpp"
#include <algorithm>
#include <climits>
#include <type_traits>
#include <utility>
#include <vector>

using namespace gemhip;

namespace {

constexpr int EV_BLOCK = 256;
constexpr int EV_NREG = EV_MAXNB / WAVE;       // EV_MAXNB (eval_host.hpp) true neighbours per chunk, held in registers

template <int KIND>
__device__ __forceinline__ double finish_score(double sum)      // sum: the fp64 dot (kind 0) or the fp64 squared distance (kind 1)
{
    if (KIND == 0) return sum;
    const double r = sqrt(sum);                                  // lap.py:74  exp(-power(norm(x_i - x_j), 2))
    return exp(-(r * r));
}

template <int KIND>
__device__ __forceinline__ double term(float a, float b)
{
    if (KIND == 0) return (double)a * (double)b;
    const double t = (double)a - (double)b;
    return t * t;
}

// ---- link prediction: the handle's CSR is the TEST graph, a second CSR (the TRAIN graph, rows sorted and de-duplicated by
// gemhip_eval_set_mask) removes candidates: j is a candidate of i only if (i -> j) is not a training arc.  A wavefront visits its j in
// ascending order, so it walks ONE cursor through the sorted mask row of i -- the row stays in global memory, however long (a hub's
// training neighbours), and the entry under the cursor is kept in a register: a row that is not masked costs one integer compare.
struct MaskWalk {
    const int32_t *p, *end; int cur;                               // cur = *p, or INT_MAX past the end (every j is < n <= INT_MAX)
    __device__ __forceinline__ void open(const int64_t *__restrict__ mask_row_ptr, const int32_t *__restrict__ mask_col, int i, int64_t first)
    {
        p = end = nullptr; cur = INT_MAX;
        if (!mask_row_ptr) return;
        const int32_t *lo = mask_col + mask_row_ptr[i], *hi = mask_col + mask_row_ptr[i + 1];
        end = hi;
        while (lo < hi) { const int32_t *mid = lo + ((hi - lo) >> 1); if (*mid < first) lo = mid + 1; else hi = mid; }     // entries below `first` are never asked for
        p = lo; cur = p < end ? *p : INT_MAX;
    }
    __device__ __forceinline__ bool masked(int64_t j)              // j never decreases between calls
    {
        while (cur < j) { ++p; cur = p < end ? *p : INT_MAX; }
        return cur == j;
    }
};

struct NoMask { __device__ __forceinline__ bool masked(int64_t) const { return false; } };      // what an unmasked stream asks instead: nothing, no state

// A_i in registers and the fp64 score of a row of B: the one row score of the AP and top-k kernels.
template <int NV, int KIND>     // lane l holds columns (c*64 + l), c < NV  (da <= 64*NV)
struct RowScore {
    float a[NV]; const float *B; int ldb, da, lane;
    __device__ __forceinline__ RowScore(const float *__restrict__ A, const float *__restrict__ B_, int ldb_, int da_, int i) : B(B_), ldb(ldb_), da(da_), lane(lane_id())
    {
#pragma unroll
        for (int c = 0; c < NV; ++c) { const int cc = c * WAVE + lane; a[c] = cc < da ? A[(int64_t)i * ldb + cc] : 0.f; }
    }
    __device__ __forceinline__ double operator()(int64_t j) const
    {
        double part = 0.0;
        const float *bj = B + j * ldb;
#pragma unroll
        for (int c = 0; c < NV; ++c) { const int cc = c * WAVE + lane; if (cc < da) part += term<KIND>(a[c], bj[cc]); }
        return finish_score<KIND>(wave_sum_f64(part));
    }
};

// The AP kernel.  One workgroup per (sampled node, chunk of <= EV_MAXNB of its positives): hubs of a power-law graph take several chunks.
// MASKED: the mask is applied in the stream -- the chunks hold the POSITIVES of i (its test neighbours that are not masked; the host removes the
// masked ones), and rank_all counts unmasked candidates only.  Without it no MaskWalk exists (NoMask stands in) and the mask arguments are not read.
template <int NV, int KIND, bool MASKED>
__global__ __launch_bounds__(EV_BLOCK) void eval_ap_kernel(int64_t n, int da, const float *__restrict__ A, const float *__restrict__ B, int ldb,
                                                           int undirected, const int32_t *__restrict__ chunk_node, const int64_t *__restrict__ chunk_off,
                                                           const int32_t *__restrict__ chunk_cnt, const int32_t *__restrict__ nb,
                                                           const int64_t *__restrict__ mask_row_ptr, const int32_t *__restrict__ mask_col,
                                                           double *__restrict__ s_out, int32_t *__restrict__ cnt_out)
{
    __shared__ double s_nb[EV_MAXNB];
    __shared__ int t_nb[EV_MAXNB];
    __shared__ int cnt_nb[EV_MAXNB];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // in a scalar register: j and the mask cursor stay scalar
    const int i = chunk_node[blockIdx.x];
    const int64_t off = chunk_off[blockIdx.x];
    const int nnb = chunk_cnt[blockIdx.x];
    for (int k = threadIdx.x; k < EV_MAXNB; k += EV_BLOCK) { cnt_nb[k] = 0; t_nb[k] = k < nnb ? nb[off + k] : -1; }
    __syncthreads();
    const RowScore<NV, KIND> score(A, B, ldb, da, i);
    for (int k = wave; k < nnb; k += EV_BLOCK / WAVE) {
        const double s = score(t_nb[k]);
        if (lane == 0) s_nb[k] = s;
    }
    __syncthreads();
    double my_s[EV_NREG]; int my_t[EV_NREG]; int my_c[EV_NREG];
#pragma unroll
    for (int r = 0; r < EV_NREG; ++r) {
        const int k = r * WAVE + lane;
        my_s[r] = k < nnb ? s_nb[k] : 0.0; my_t[r] = k < nnb ? t_nb[k] : -1; my_c[r] = 0;
    }
    // ---- stream the candidates (j != i, and j > i when undirected: evaluation_util.py:28-35; not a mask arc)
    const int64_t lo = undirected ? (int64_t)i + 1 : 0;
    const int nreg_used = (nnb + WAVE - 1) / WAVE;
    std::conditional_t<MASKED, MaskWalk, NoMask> mask;
    if constexpr (MASKED) mask.open(mask_row_ptr, mask_col, i, lo);
    for (int64_t j = lo + wave; j < n; j += EV_BLOCK / WAVE) {
        if (j == i || mask.masked(j)) continue;
        const double s = score(j);
        if (!(s > 0.0)) continue;                                  // evaluation_util.py:34  adj[i, j] > threshold (0.0)
#pragma unroll
        for (int r = 0; r < EV_NREG; ++r)
            if (r < nreg_used) my_c[r] += (s > my_s[r] || (s == my_s[r] && j < my_t[r])) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < EV_NREG; ++r) {
        const int k = r * WAVE + lane;
        if (k < nnb && my_c[r]) atomicAdd(&cnt_nb[k], my_c[r]);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nnb; k += EV_BLOCK) { s_out[off + k] = s_nb[k]; cnt_out[off + k] = cnt_nb[k]; }
}

// Is (i -> j) an arc of the CSR: bisects row i, whose columns are ascending.
__device__ __forceinline__ bool csr_has_arc(const int64_t *row_ptr, const int32_t *col, int i, int j)
{
    int64_t hi = row_ptr[i + 1], lo = row_ptr[i];
    const int64_t end = hi;
    while (lo < hi) { const int64_t mid = lo + ((hi - lo) >> 1); if (col[mid] < j) lo = mid + 1; else hi = mid; }
    return lo < end && col[lo] == j;
}

// ---- per-node top-k: one workgroup per sampled node, the same row stream and mask walk.  Every wavefront keeps the k best of the rows IT
// saw, unsorted, in its own slice of LDS (12 k bytes; 48 KiB per workgroup at k = 1024, three workgroups per CU), behind a running threshold:
// the entry that ranks LAST among the kept ones.  Lane l owns slots l, l + 64, ... and keeps the last-ranked of its own slots in registers, so a
// row below the threshold costs one compare, and a row that enters replaces the threshold entry: the owner rescans its <= 16 slots, one butterfly
// finds the new threshold.  The order is total (score descending, node id ascending; ids are distinct), so the k best of the union of the four
// lists are the node's k best, and each entry's place is the number of entries that rank before it -- counted, not sorted: no atomics, and
// the same bytes whatever the wavefronts' timing.  Only k values per wavefront are ever held: no nsample x n matrix.
constexpr int TK_MAXK = 1024;
constexpr int TK_WAVES = EV_BLOCK / WAVE;

__device__ __forceinline__ bool ranks_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// The last-ranked of the lanes' (s, id, slot); slot < 0: the lane holds nothing.  Every lane ends with the same triple.
__device__ __forceinline__ void wave_last_ranked(double &s, int &id, int &slot)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double os = __shfl_xor(s, o); const int oi = __shfl_xor(id, o), osl = __shfl_xor(slot, o);
        if (osl >= 0 && (slot < 0 || ranks_before(s, id, os, oi))) { s = os; id = oi; slot = osl; }
    }
}

template <int NV, int KIND>
__global__ __launch_bounds__(EV_BLOCK) void eval_topk_kernel(int64_t n, int da, const float *__restrict__ A, const float *__restrict__ B, int ldb, int undirected,
                                                             const int32_t *__restrict__ nodes, int k, const int64_t *__restrict__ mask_row_ptr,
                                                             const int32_t *__restrict__ mask_col, const int64_t *__restrict__ row_ptr,
                                                             const int32_t *__restrict__ col, int32_t *__restrict__ id_out, double *__restrict__ score_out,
                                                             uint8_t *__restrict__ hit_out)
{
    extern __shared__ double tk_lds[];                             // [TK_WAVES][k] scores, then [TK_WAVES][k] ids
    __shared__ int w_cnt[TK_WAVES];
    double *const s_all = tk_lds; int *const id_all = reinterpret_cast<int *>(tk_lds + TK_WAVES * k);
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);       // in a scalar register: j and the mask cursor stay scalar
    const int i = nodes[blockIdx.x];
    double *const ls = s_all + wave * k; int *const li = id_all + wave * k;
    const RowScore<NV, KIND> score(A, B, ldb, da, i);
    const int64_t lo = undirected ? (int64_t)i + 1 : 0;
    MaskWalk mask;
    mask.open(mask_row_ptr, mask_col, i, lo);
    int cnt = 0;                                                   // kept entries of this wavefront (wave-uniform)
    double my_s = 0.0; int my_id = -1, my_slot = -1;               // the last-ranked of this lane's own slots
    double th_s = 0.0; int th_id = -1, th_slot = -1;               // the wavefront's threshold entry, valid once cnt == k
    for (int64_t j = lo + wave; j < n; j += TK_WAVES) {
        if (j == i || mask.masked(j)) continue;
        const double s = score(j);
        if (!(s > 0.0)) continue;
        if (cnt < k) {
            if (lane == (cnt & (WAVE - 1))) {
                ls[cnt] = s; li[cnt] = (int)j;
                if (my_slot < 0 || ranks_before(my_s, my_id, s, (int)j)) { my_s = s; my_id = (int)j; my_slot = cnt; }
            }
            if (++cnt == k) { th_s = my_s; th_id = my_id; th_slot = my_slot; wave_last_ranked(th_s, th_id, th_slot); }
            continue;
        }
        if (!ranks_before(s, (int)j, th_s, th_id)) continue;
        if (lane == (th_slot & (WAVE - 1))) {
            ls[th_slot] = s; li[th_slot] = (int)j;
            my_slot = -1;
            for (int q = lane; q < k; q += WAVE) {
                const double qs = ls[q]; const int qi = li[q];
                if (my_slot < 0 || ranks_before(my_s, my_id, qs, qi)) { my_s = qs; my_id = qi; my_slot = q; }
            }
        }
        th_s = my_s; th_id = my_id; th_slot = my_slot;
        wave_last_ranked(th_s, th_id, th_slot);
    }
    if (lane == 0) w_cnt[wave] = cnt;
    __syncthreads();
    // ---- merge: the place of an entry = the number of kept entries (all wavefronts) that rank before it
    int total = 0;
    for (int w = 0; w < TK_WAVES; ++w) total += w_cnt[w];
    const int64_t out = (int64_t)blockIdx.x * k;
    for (int e = threadIdx.x; e < TK_WAVES * k; e += EV_BLOCK) {
        const int w = e / k;
        if (e - w * k >= w_cnt[w]) continue;
        const double s = s_all[e]; const int id = id_all[e];
        int rank = 0;
        for (int w2 = 0; w2 < TK_WAVES; ++w2) {
            const double *s2 = s_all + w2 * k; const int *id2 = id_all + w2 * k;
            const int c2 = w_cnt[w2];
            for (int q = 0; q < c2; ++q) rank += ranks_before(s2[q], id2[q], s, id) ? 1 : 0;
        }
        if (rank >= k) continue;
        const bool hit = csr_has_arc(row_ptr, col, i, id);         // is (i -> id) a test arc
        id_out[out + rank] = id; score_out[out + rank] = s; hit_out[out + rank] = hit ? 1 : 0;
    }
    for (int r = (total < k ? total : k) + threadIdx.x; r < k; r += EV_BLOCK) { id_out[out + r] = -1; score_out[out + r] = 0.0; hit_out[out + r] = 0; }
}

// ---- pair scoring: a 16-lane group per (st, ed); one row of A and one of B are gathered per pair (2*4*d bytes), nothing is reused, so the kernel
// is a pure row gather.  Four pairs per wavefront keep all 64 lanes busy at d <= 64 and four times as many rows in flight as a wavefront per pair.
// VEC (ld % 4 == 0: every row starts on 16 bytes): lane s of the group loads the float4 at columns 4*(16c + s), c < NV; the tail float4 of a row
// with da % 4 != 0 stays inside the row's ld and its surplus elements are masked.  Otherwise lane s reads columns 64c + 16k + s one by one.
// Each lane sums its terms in column order in fp64, then the 16 partial sums are folded by a fixed butterfly: no atomics, the same bits every run.
constexpr int EP_BLOCK = 256;
constexpr int EP_GROUP = 16;
constexpr int EP_MAX_BLOCKS = 256 * 16;         // 16 workgroups per CU; further pairs are taken by the grid-stride loop

template <int KIND, bool VEC, int NV>           // da <= 64*NV
__global__ __launch_bounds__(EP_BLOCK) void eval_pairs_kernel(int da, int ld, const float *__restrict__ A, const float *__restrict__ B,
                                                              const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, int64_t npairs,
                                                              const int32_t *__restrict__ st, const int32_t *__restrict__ ed,
                                                              double *__restrict__ score_out, uint8_t *__restrict__ hit_out)
{
    const int sub = threadIdx.x & (EP_GROUP - 1);
    const int64_t ngroups = (int64_t)gridDim.x * (EP_BLOCK / EP_GROUP);
    for (int64_t p = ((int64_t)blockIdx.x * EP_BLOCK + threadIdx.x) / EP_GROUP; p < npairs; p += ngroups) {      // uniform within a group
        const int i = st[p], j = ed[p];
        const float *a = A + (int64_t)i * ld, *b = B + (int64_t)j * ld;
        double part = 0.0;
        if (VEC) {
            float4 va[NV], vb[NV];
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const int cc = (c * EP_GROUP + sub) * 4;
                va[c] = cc < da ? *reinterpret_cast<const float4 *>(a + cc) : make_float4(0.f, 0.f, 0.f, 0.f);
                vb[c] = cc < da ? *reinterpret_cast<const float4 *>(b + cc) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                const int cc = (c * EP_GROUP + sub) * 4;
                if (cc < da) part += term<KIND>(va[c].x, vb[c].x);
                if (cc + 1 < da) part += term<KIND>(va[c].y, vb[c].y);
                if (cc + 2 < da) part += term<KIND>(va[c].z, vb[c].z);
                if (cc + 3 < da) part += term<KIND>(va[c].w, vb[c].w);
            }
        } else {
#pragma unroll
            for (int c = 0; c < NV; ++c) {
                float sa[4], sb[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int cc = c * 64 + k * EP_GROUP + sub;
                    sa[k] = cc < da ? a[cc] : 0.f; sb[k] = cc < da ? b[cc] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) if (c * 64 + k * EP_GROUP + sub < da) part += term<KIND>(sa[k], sb[k]);
            }
        }
#pragma unroll
        for (int o = EP_GROUP / 2; o >= 1; o >>= 1) part += __shfl_xor(part, o);       // partners stay inside the group, which is all active or all idle
        if (sub == 0) {
            score_out[p] = i == j ? 0.0 : finish_score<KIND>(part);                   // zero diagonal of get_reconstructed_adj
            if (hit_out) hit_out[p] = csr_has_arc(row_ptr, col, i, j) ? 1 : 0;        // true_digraph.has_edge(st, ed): directed
        }
    }
}

// ---- host side
// Runs `launch` between two marks on the null stream, waits for it and stores the device time in *ms.
template <typename Launch>
hipError_t timed_launch(double *ms, Launch launch)
{
    Stopwatch t;
    hipError_t e = start(t);
    if (e != hipSuccess) return e;
    launch();
    e = hipGetLastError();
    return e != hipSuccess ? e : stop(t, ms);
}

// The one map from a handle's (kind, da) to the kernels' compile-time <NV, KIND>: f(integral_constant NV, integral_constant KIND).
template <typename F>
void dispatch_width(int kind, int da, F f)
{
    auto with_nv = [&](auto NV) {
        if (kind == 0) f(NV, std::integral_constant<int, 0>{}); else f(NV, std::integral_constant<int, 1>{});
    };
    const int nv = (da + WAVE - 1) / WAVE;
    if (nv <= 1) with_nv(std::integral_constant<int, 1>{});
    else if (nv <= 2) with_nv(std::integral_constant<int, 2>{});
    else if (nv <= 4) with_nv(std::integral_constant<int, 4>{});
    else with_nv(std::integral_constant<int, 8>{});
}

// The refusal of a CSR that check_eval_csr did not pass, in the words of `who`.
int refuse_csr(const char *who, const EvalCsrError &err, int64_t n, const int64_t *row_ptr)
{
    switch (err.kind) {
    case EvalCsrError::ROW_PTR_FIRST: return fail(GEMHIP_E_INVALID, "%s: row_ptr[0] is %lld, not 0", who, (long long)row_ptr[0]);
    case EvalCsrError::ROW_PTR_DECREASES: return fail(GEMHIP_E_INVALID, "%s: row_ptr decreases at row %lld", who, (long long)err.index);
    case EvalCsrError::COL_NULL: return fail(GEMHIP_E_INVALID, "%s: col is null", who);
    default: return fail(GEMHIP_E_INVALID, "%s: column %d outside [0,%lld)", who, err.column, (long long)n);
    }
}

}  // namespace

struct gemhip_eval {
    int64_t n = 0, nnz = 0; int da = 0, ld = 0, kind = 0; bool cols_sorted = true; int dev = 0;
    std::vector<int64_t> row_ptr; std::vector<int32_t> col;          // host copy: the AP call cuts the sampled nodes' rows into chunks
    DevBuf<float> A, B; DevBuf<int64_t> d_row_ptr; DevBuf<int32_t> d_col;
    DevBuf<int32_t> d_st, d_ed; DevBuf<double> d_score; DevBuf<uint8_t> d_hit;     // pair scratch, grow-only
    bool has_mask = false;                                           // link prediction: the train graph, rows sorted and de-duplicated
    EvalMask mask;
    DevBuf<int64_t> d_mask_row_ptr; DevBuf<int32_t> d_mask_col;
    double last_pairs_ms = 0.0, last_kernel_ms = 0.0;
    const float *dB() const { return B ? B.get() : A.get(); }
};

extern "C" int gemhip_eval_create(int64_t n, int32_t da, int32_t ld, const float *A_host, const float *B_host, int32_t kind, const int64_t *row_ptr,
                                  const int32_t *col, gemhip_eval_t *out)
{
    GEMHIP_REQUIRE(out, "eval_create: out is null");
    *out = nullptr;
    GEMHIP_REQUIRE(n >= 1 && n <= INT32_MAX && da >= 1 && da <= 512 && ld >= da && A_host && row_ptr, "eval_create: bad arguments (1 <= da <= 512, ld >= da, n < 2^31)");
    GEMHIP_REQUIRE(kind == 0 || kind == 1, "eval_create: kind %d is neither 0 (inner product) nor 1 (exp of minus squared distance)", kind);
    GEMHIP_REQUIRE(kind == 0 || !B_host || B_host == A_host, "eval_create: kind 1 scores one embedding against itself (B must be NULL)");
    bool sorted = true;
    if (const EvalCsrError err = check_eval_csr(n, row_ptr, col, &sorted)) return refuse_csr("eval_create", err, n, row_ptr);
    const int64_t nnz = row_ptr[n];
    gemhip_eval *h = new gemhip_eval;
    h->n = n; h->nnz = nnz; h->da = da; h->ld = ld; h->kind = kind; h->cols_sorted = sorted;
    h->row_ptr.assign(row_ptr, row_ptr + n + 1);
    if (nnz) h->col.assign(col, col + nnz);
    hipError_t e = hipGetDevice(&h->dev);
    if (e == hipSuccess) e = h->A.upload(A_host, (size_t)n * ld);
    if (e == hipSuccess && B_host && B_host != A_host) e = h->B.upload(B_host, (size_t)n * ld);
    if (e == hipSuccess) e = h->d_row_ptr.upload(row_ptr, (size_t)n + 1);
    if (e == hipSuccess) e = h->d_col.upload(col, (size_t)nnz);
    if (e != hipSuccess) { delete h; return fail(GEMHIP_E_HIP, "eval_create: %s", hipGetErrorString(e)); }
    *out = h;
    return GEMHIP_OK;
}

extern "C" int gemhip_eval_destroy(gemhip_eval_t h)
{
    delete h;
    return GEMHIP_OK;
}

namespace {

// gemhip_eval_ap (masked = false: the handle's mask is ignored) and gemhip_eval_ap_masked: validate, ap_chunks, upload, launch, download, ap_from_counts.
int ap_impl(gemhip_eval_t h, const char *who, bool masked, int32_t undirected, int64_t nsample, const int32_t *nodes, double *ap_out, int64_t *npos_out)
{
    GEMHIP_REQUIRE(h && nsample >= 0 && (nsample == 0 || (nodes && ap_out)), "%s: bad arguments", who);
    if (nsample == 0) return GEMHIP_OK;
    const int64_t n = h->n;
    const int64_t bad = first_bad_index(nodes, nsample, n);
    GEMHIP_REQUIRE(bad < 0, "%s: node %d outside [0,%lld)", who, nodes[bad], (long long)n);
    const bool use_mask = masked && h->has_mask;
    const ApChunks c = ap_chunks(h->row_ptr.data(), h->col.data(), use_mask ? h->mask.row_ptr.data() : nullptr, use_mask ? h->mask.col.data() : nullptr,
                                 undirected != 0, nsample, nodes);
    const int64_t nchunk = (int64_t)c.chunk_node.size(), total = (int64_t)c.nb.size();
    std::vector<double> s_host(std::max<int64_t>(total, 1)); std::vector<int32_t> cnt_host(std::max<int64_t>(total, 1));
    h->last_kernel_ms = 0.0;
    if (nchunk > 0) {
        DevBuf<int32_t> dnb, dcn, dcc, dcnt; DevBuf<int64_t> dco; DevBuf<double> ds;
        GEMHIP_CHECK(dnb.upload(c.nb.data(), total));
        GEMHIP_CHECK(dcn.upload(c.chunk_node.data(), nchunk));
        GEMHIP_CHECK(dcc.upload(c.chunk_cnt.data(), nchunk));
        GEMHIP_CHECK(dco.upload(c.chunk_off.data(), nchunk));
        GEMHIP_CHECK(ds.reserve(total)); GEMHIP_CHECK(dcnt.reserve(total));
        auto launch = [&](auto NV, auto KIND, auto MASKED) {
            hipLaunchKernelGGL((eval_ap_kernel<decltype(NV)::value, decltype(KIND)::value, decltype(MASKED)::value>), dim3((unsigned)nchunk), dim3(EV_BLOCK), 0, 0,
                               n, h->da, h->A.get(), h->dB(), h->ld, (int)undirected, dcn.get(), dco.get(), dcc.get(), dnb.get(), h->d_mask_row_ptr.get(),
                               h->d_mask_col.get(), ds.get(), dcnt.get());
        };
        GEMHIP_CHECK(timed_launch(&h->last_kernel_ms, [&] {
            dispatch_width(h->kind, h->da, [&](auto NV, auto KIND) { if (use_mask) launch(NV, KIND, std::true_type{}); else launch(NV, KIND, std::false_type{}); });
        }));
        GEMHIP_CHECK(hipMemcpy(s_host.data(), ds, total * 8, hipMemcpyDeviceToHost));
        GEMHIP_CHECK(hipMemcpy(cnt_host.data(), dcnt, total * 4, hipMemcpyDeviceToHost));
    }
    ap_from_counts(nsample, c.nb.data(), c.node_off.data(), s_host.data(), cnt_host.data(), ap_out, npos_out);
    return GEMHIP_OK;
}

}  // namespace

extern "C" int gemhip_eval_ap(gemhip_eval_t h, int32_t undirected, int64_t nsample, const int32_t *nodes, double *ap_out)
{
    return ap_impl(h, "eval_ap", false, undirected, nsample, nodes, ap_out, nullptr);
}

extern "C" int gemhip_eval_set_mask(gemhip_eval_t h, const int64_t *mask_row_ptr, const int32_t *mask_col)
{
    GEMHIP_REQUIRE(h, "eval_set_mask: handle is null");
    if (!mask_row_ptr) {                                             // clear
        h->has_mask = false;
        h->mask = EvalMask();
        h->d_mask_row_ptr.reset(); h->d_mask_col.reset();
        return GEMHIP_OK;
    }
    if (const EvalCsrError err = check_eval_csr(h->n, mask_row_ptr, mask_col, nullptr)) return refuse_csr("eval_set_mask", err, h->n, mask_row_ptr);
    EvalMask m = normalise_mask(h->n, mask_row_ptr, mask_col);       // the kernels walk a cursor through a row: ascending, each column once
    DevBuf<int64_t> drp; DevBuf<int32_t> dcl;                        // uploaded first: a failed copy leaves the handle's mask as it was
    GEMHIP_CHECK(drp.upload(m.row_ptr.data(), m.row_ptr.size()));
    GEMHIP_CHECK(dcl.upload(m.col.data(), m.col.size()));
    h->d_mask_row_ptr = std::move(drp); h->d_mask_col = std::move(dcl);
    h->mask = std::move(m);
    h->has_mask = true;
    return GEMHIP_OK;
}

extern "C" int gemhip_eval_ap_masked(gemhip_eval_t h, int32_t undirected, int64_t nsample, const int32_t *nodes, double *ap_out, int64_t *npos_out)
{
    return ap_impl(h, "eval_ap_masked", true, undirected, nsample, nodes, ap_out, npos_out);
}

extern "C" int gemhip_eval_topk(gemhip_eval_t h, int32_t undirected, int32_t use_mask, int64_t nsample, const int32_t *nodes, int32_t k, int32_t *id_out,
                                double *score_out, uint8_t *hit_out)
{
    GEMHIP_REQUIRE(h && nsample >= 0 && nsample <= INT32_MAX && (nsample == 0 || (nodes && id_out && score_out && hit_out)), "eval_topk: bad arguments");
    GEMHIP_REQUIRE(k >= 1 && k <= TK_MAXK, "eval_topk: k = %d outside [1,%d]", k, TK_MAXK);
    GEMHIP_REQUIRE(h->cols_sorted, "eval_topk: the edge lookup needs every CSR row's columns in ascending order");
    if (nsample == 0) return GEMHIP_OK;
    const int64_t n = h->n;
    const int64_t bad = first_bad_index(nodes, nsample, n);
    GEMHIP_REQUIRE(bad < 0, "eval_topk: node %d outside [0,%lld)", nodes[bad], (long long)n);
    const bool masked = use_mask && h->has_mask;
    const int64_t *dmrp = masked ? h->d_mask_row_ptr.get() : nullptr; const int32_t *dmcol = masked ? h->d_mask_col.get() : nullptr;
    DevBuf<int32_t> dnodes, did; DevBuf<double> dscore; DevBuf<uint8_t> dhit;
    const size_t total = (size_t)nsample * (size_t)k;
    GEMHIP_CHECK(dnodes.upload(nodes, nsample));
    GEMHIP_CHECK(did.reserve(total)); GEMHIP_CHECK(dscore.reserve(total)); GEMHIP_CHECK(dhit.reserve(total));
    const size_t lds = (size_t)TK_WAVES * k * (sizeof(double) + sizeof(int));
    GEMHIP_CHECK(timed_launch(&h->last_kernel_ms, [&] {
        dispatch_width(h->kind, h->da, [&](auto NV, auto KIND) {
            hipLaunchKernelGGL((eval_topk_kernel<decltype(NV)::value, decltype(KIND)::value>), dim3((unsigned)nsample), dim3(EV_BLOCK), lds, 0, n, h->da, h->A.get(),
                               h->dB(), h->ld, (int)undirected, dnodes.get(), (int)k, dmrp, dmcol, h->d_row_ptr.get(), h->d_col.get(), did.get(), dscore.get(),
                               dhit.get());
        });
    }));
    GEMHIP_CHECK(hipMemcpy(id_out, did, total * sizeof(int32_t), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(score_out, dscore, total * sizeof(double), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(hit_out, dhit, total, hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_eval_last_kernel_ms(gemhip_eval_t h, double *ms_out)
{
    GEMHIP_REQUIRE(h && ms_out, "eval_last_kernel_ms: bad arguments");
    *ms_out = h->last_kernel_ms;
    return GEMHIP_OK;
}

extern "C" int gemhip_eval_pairs(gemhip_eval_t h, int64_t npairs, const int32_t *st, const int32_t *ed, double *score_out, uint8_t *hit_out)
{
    GEMHIP_REQUIRE(h && npairs >= 0 && (npairs == 0 || (st && ed && score_out)), "eval_pairs: bad arguments");
    if (npairs == 0) return GEMHIP_OK;
    GEMHIP_REQUIRE(!hit_out || h->cols_sorted, "eval_pairs: the edge lookup needs every CSR row's columns in ascending order");
    for (int64_t p = 0; p < npairs; ++p) {
        GEMHIP_REQUIRE(st[p] >= 0 && st[p] < h->n, "eval_pairs: st[%lld] = %d outside [0,%lld)", (long long)p, st[p], (long long)h->n);
        GEMHIP_REQUIRE(ed[p] >= 0 && ed[p] < h->n, "eval_pairs: ed[%lld] = %d outside [0,%lld)", (long long)p, ed[p], (long long)h->n);
    }
    GEMHIP_CHECK(h->d_st.upload(st, npairs));
    GEMHIP_CHECK(h->d_ed.upload(ed, npairs));
    GEMHIP_CHECK(h->d_score.reserve(npairs));
    if (hit_out) GEMHIP_CHECK(h->d_hit.reserve(npairs));
    const unsigned blocks = (unsigned)std::min<int64_t>((npairs + EP_BLOCK / EP_GROUP - 1) / (EP_BLOCK / EP_GROUP), EP_MAX_BLOCKS);
    uint8_t *dhit = hit_out ? h->d_hit.get() : nullptr;
    auto launch = [&](auto NV, auto KIND, auto VEC) {
        hipLaunchKernelGGL((eval_pairs_kernel<decltype(KIND)::value, decltype(VEC)::value, decltype(NV)::value>), dim3(blocks), dim3(EP_BLOCK), 0, 0, h->da, h->ld,
                           h->A.get(), h->dB(), h->d_row_ptr.get(), h->d_col.get(), npairs, h->d_st.get(), h->d_ed.get(), h->d_score.get(), dhit);
    };
    GEMHIP_CHECK(timed_launch(&h->last_pairs_ms, [&] {
        dispatch_width(h->kind, h->da, [&](auto NV, auto KIND) { if (h->ld % 4 == 0) launch(NV, KIND, std::true_type{}); else launch(NV, KIND, std::false_type{}); });
    }));
    GEMHIP_CHECK(hipMemcpy(score_out, h->d_score, npairs * 8, hipMemcpyDeviceToHost));
    if (hit_out) GEMHIP_CHECK(hipMemcpy(hit_out, h->d_hit, npairs, hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_eval_last_pairs_ms(gemhip_eval_t h, double *ms_out)
{
    GEMHIP_REQUIRE(h && ms_out, "eval_last_pairs_ms: bad arguments");
    *ms_out = h->last_pairs_ms;
    return GEMHIP_OK;
}

// One-shot form of create + ap + destroy for inner-product scores (kind 0).
extern "C" int gemhip_eval_sampled_ap(int64_t n, int32_t da, int32_t ld, const float *A_host, const float *B_host, const int64_t *row_ptr,
                                      const int32_t *col, int32_t undirected, int64_t nsample, const int32_t *nodes, double *ap_out)
{
    GEMHIP_REQUIRE(n >= 1 && da >= 1 && da <= 512 && ld >= da && A_host && row_ptr && nsample >= 0 && (nsample == 0 || (nodes && ap_out)),
                   "eval_sampled_ap: bad arguments (da <= 512)");
    if (nsample == 0) return GEMHIP_OK;
    const int64_t bad = first_bad_index(nodes, nsample, n);
    GEMHIP_REQUIRE(bad < 0, "eval_sampled_ap: node %d outside [0,%lld)", nodes[bad], (long long)n);
    gemhip_eval_t h = nullptr;
    int rc = gemhip_eval_create(n, da, ld, A_host, B_host, 0, row_ptr, col, &h);
    if (rc != GEMHIP_OK) return rc;
    rc = gemhip_eval_ap(h, undirected, nsample, nodes, ap_out);
    gemhip_eval_destroy(h);
    return rc;
}
