// nbr.hip -- the neighbourhood link-prediction baselines: common neighbours, Jaccard's coefficient, Adamic-Adar, resource
// allocation and preferential attachment of node pairs on the simple undirected graph of an arc list -- the first rows of the node2vec
// paper's table 4, which networkx computes with a Python loop per pair.
//
// Kernels
//   nbr_score_kernel<G>  one work item (a slice of the shorter neighbour list a of a pair, nbr_host.hpp) per group of G lanes: each lane takes
//                        elements of the slice, strided, and binary-searches each in the longer list b; on a hit it counts one and gathers
//                        w_aa[x] and w_ra[x] into two fp64 sums, in ascending order of its own elements; the group adds its lanes by a
//                        butterfly.  G = 16 for narrow items (four per wave), G = 64 for wide ones.  An unsplit pair finishes in place
//                        (jaccard and pa from the degrees); a slice of a split pair writes its partial slot.
//   nbr_finish_kernel    adds the partials of a split pair in slice order and finishes it.
// The outputs are zeroed first: a pair with an empty list has no item, and all of its five scores are zero.
//
// Numerics.  cn is an integer; jaccard is one fp64 division of two integers and pa one fp64 product of two converted integers (no fast-math:
// both correctly rounded, bit-equal to numpy's).  The fp64 sums have no atomics and an order that is a function of the two lists alone, so the
// bytes are the same on every run and for both orientations of a pair.  The weight tables are made on the host (nbr_host.hip) and only
// gathered here; gemhip_nbr_weights reads them back from the device.
//
// Every refusal is decided on the host before any device call: nbr_host.hip finds the offender, this file words it.
#include "eval_common.hpp"
#include "nbr_host.hpp"
#include <algorithm>
#include <memory>
#include <vector>

using namespace gemhip;

struct gemhip_nbr {
    int64_t n = 0, nnz = 0, max_deg = 0;
    std::vector<int32_t> deg;                                // host copy: the planner reads it
    DevBuf<int64_t> row_ptr;
    DevBuf<int32_t> col, d_deg;
    DevBuf<double> w_aa, w_ra;
    DevBuf<int32_t> st, ed, cn, part_cn;
    DevBuf<double> jac, aa, ra, pa, part_aa, part_ra;
    DevBuf<NbrItem> narrow, wide;
    DevBuf<NbrSplit> split;
    Stopwatch watch;
    double ms[6] = {0, 0, 0, 0, 0, 0};                       // ingest, graph upload, plan, pair and item upload, kernels, download
    int64_t last[6] = {0, 0, 0, 0, 0, 0};                    // of the last call: narrow items, wide items, split pairs, slots, longest item, m
};

namespace {

constexpr int NBR_THREADS = 256;
constexpr int NBR_MAX_GRID = 8192;

template <int G>
__global__ __launch_bounds__(NBR_THREADS) void nbr_score_kernel(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
                                                                const int32_t *__restrict__ deg, const double *__restrict__ w_aa,
                                                                const double *__restrict__ w_ra, const int32_t *__restrict__ st,
                                                                const int32_t *__restrict__ ed, const NbrItem *__restrict__ items, int64_t n_items,
                                                                int32_t *__restrict__ cn, double *__restrict__ jac, double *__restrict__ aa,
                                                                double *__restrict__ ra, double *__restrict__ pa, int32_t *__restrict__ part_cn,
                                                                double *__restrict__ part_aa, double *__restrict__ part_ra)
{
    constexpr int PER_WAVE = WAVE / G;
    const int lane = threadIdx.x & (WAVE - 1), sub = lane / G, gl = lane % G;
    const int64_t wave = (int64_t)blockIdx.x * (NBR_THREADS / WAVE) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (NBR_THREADS / WAVE);
    // The trip count is the wave's, not the group's: a group without an item runs the butterfly with zeros, it never leaves early.
    for (int64_t base = wave * PER_WAVE; base < n_items; base += nwaves * PER_WAVE) {
        const int64_t it = base + sub;
        const bool live = it < n_items;
        int32_t hits = 0, du = 0, dv = 0;
        double s_aa = 0.0, s_ra = 0.0;
        NbrItem item = {0, 0, 0, -1};
        if (live) {
            item = items[it];
            const int32_t u = st[item.pair], v = ed[item.pair];
            du = deg[u]; dv = deg[v];
            const bool first = nbr_first_is_a(du, dv, u, v);
            const int32_t lb = first ? dv : du;
            const int32_t *A = col + (row_ptr[first ? u : v] + (int64_t)item.start);       // int64 offsets into col
            const int32_t *B = col + row_ptr[first ? v : u];
            for (int32_t k = gl; k < item.len; k += G) {
                const int32_t x = A[k];
                int32_t lo = 0, hi = lb;                                                    // lower bound of x in B[0, lb)
                while (lo < hi) {
                    const int32_t mid = lo + ((hi - lo) >> 1);
                    if (B[mid] < x) lo = mid + 1; else hi = mid;
                }
                if (lo < lb && B[lo] == x) {
                    ++hits;
                    s_aa += w_aa[x];
                    s_ra += w_ra[x];
                }
            }
        }
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {               // o < G: lane ^ o stays inside the group
            hits += __shfl_xor(hits, o);
            s_aa += __shfl_xor(s_aa, o);
            s_ra += __shfl_xor(s_ra, o);
        }
        if (live && gl == 0) {
            if (item.slot < 0) {
                cn[item.pair] = hits;
                jac[item.pair] = (double)hits / (double)((int64_t)du + (int64_t)dv - (int64_t)hits);   // la >= 1: the union is not empty
                aa[item.pair] = s_aa;
                ra[item.pair] = s_ra;
                pa[item.pair] = (double)du * (double)dv;
            } else {
                part_cn[item.slot] = hits;
                part_aa[item.slot] = s_aa;
                part_ra[item.slot] = s_ra;
            }
        }
    }
}

__global__ __launch_bounds__(NBR_THREADS) void nbr_finish_kernel(const int32_t *__restrict__ deg, const int32_t *__restrict__ st, const int32_t *__restrict__ ed,
                                                                 const NbrSplit *__restrict__ split, int64_t n_split, const int32_t *__restrict__ part_cn,
                                                                 const double *__restrict__ part_aa, const double *__restrict__ part_ra, int32_t *__restrict__ cn,
                                                                 double *__restrict__ jac, double *__restrict__ aa, double *__restrict__ ra, double *__restrict__ pa)
{
    for (int64_t t = (int64_t)blockIdx.x * NBR_THREADS + threadIdx.x; t < n_split; t += (int64_t)gridDim.x * NBR_THREADS) {
        const NbrSplit sp = split[t];
        int32_t hits = 0;
        double s_aa = 0.0, s_ra = 0.0;
        for (int32_t k = 0; k < sp.n_slots; ++k) {           // slice order
            hits += part_cn[sp.first_slot + k];
            s_aa += part_aa[sp.first_slot + k];
            s_ra += part_ra[sp.first_slot + k];
        }
        const int32_t du = deg[st[sp.pair]], dv = deg[ed[sp.pair]];
        cn[sp.pair] = hits;
        jac[sp.pair] = (double)hits / (double)((int64_t)du + (int64_t)dv - (int64_t)hits);
        aa[sp.pair] = s_aa;
        ra[sp.pair] = s_ra;
        pa[sp.pair] = (double)du * (double)dv;
    }
}

unsigned nbr_grid(int64_t units, int64_t per_block) { return std::min<unsigned>(grid_of(units, per_block), NBR_MAX_GRID); }

int check_graph(const char *who, int64_t n, int64_t m, const int32_t *src, const int32_t *dst)
{
    GEMHIP_REQUIRE(n >= 1, "%s: n = %lld (need n >= 1)", who, (long long)n);
    if (n > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "%s: n = %lld: must be below 2^31", who, (long long)n);
    GEMHIP_REQUIRE(m >= 0, "%s: m = %lld arcs (need m >= 0)", who, (long long)m);
    GEMHIP_REQUIRE(m == 0 || (src && dst), "%s: NULL arc arrays", who);
    const int64_t bad = first_bad_pair(src, dst, m, n);
    GEMHIP_REQUIRE(bad < 0, "%s: arc %lld = (%d,%d) outside [0,%lld)", who, (long long)bad, src[bad], dst[bad], (long long)n);
    return GEMHIP_OK;
}

int check_pairs(const char *who, int64_t n, int64_t m, const int32_t *st, const int32_t *ed)
{
    GEMHIP_REQUIRE(m >= 1, "%s: m = %lld pairs (need m >= 1)", who, (long long)m);
    if (m > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "%s: m = %lld: must be below 2^31", who, (long long)m);
    GEMHIP_REQUIRE(st && ed, "%s: NULL pair arrays", who);
    bool self_pair = false;
    const int64_t bad = nbr_first_bad_pair(n, m, st, ed, &self_pair);
    if (bad >= 0 && self_pair)
        return fail(GEMHIP_E_INVALID, "%s: pair %lld = (%d,%d): st == ed (the scores are defined for two different nodes)", who, (long long)bad, st[bad], ed[bad]);
    GEMHIP_REQUIRE(bad < 0, "%s: pair %lld = (%d,%d) outside [0,%lld)", who, (long long)bad, st[bad], ed[bad], (long long)n);
    return GEMHIP_OK;
}

}  // namespace

extern "C" int gemhip_nbr_graph_host(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, int64_t *row_ptr_out, int32_t *col_out, int32_t *deg_out)
{
    const int rc = check_graph("nbr_graph_host", n, m, src, dst);
    if (rc) return rc;
    GEMHIP_REQUIRE(row_ptr_out && deg_out && (col_out || m == 0), "nbr_graph_host: NULL output");
    std::vector<int64_t> row_ptr;
    std::vector<int32_t> col, deg;
    nbr_build_graph(n, m, src, dst, row_ptr, col, deg);
    for (int64_t i = 0; i <= n; ++i) row_ptr_out[i] = row_ptr[i];
    for (int64_t i = 0; i < n; ++i) deg_out[i] = deg[i];
    for (size_t q = 0; q < col.size(); ++q) col_out[q] = col[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_weights_host(int64_t n, const int32_t *deg, int32_t which, double *w_out)
{
    GEMHIP_REQUIRE(n >= 1 && deg && w_out, "nbr_weights_host: n = %lld or a NULL array", (long long)n);
    GEMHIP_REQUIRE(which == 0 || which == 1, "nbr_weights_host: table %d (0 Adamic-Adar, 1 resource allocation)", which);
    for (int64_t i = 0; i < n; ++i) GEMHIP_REQUIRE(deg[i] >= 0, "nbr_weights_host: deg[%lld] = %d is negative", (long long)i, deg[i]);
    nbr_weights(n, deg, which, w_out);
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_plan_host(int64_t n, const int32_t *deg, int64_t m, const int32_t *st, const int32_t *ed, int64_t *counts_out)
{
    GEMHIP_REQUIRE(n >= 1, "nbr_plan_host: n = %lld (need n >= 1)", (long long)n);
    if (n > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "nbr_plan_host: n = %lld: must be below 2^31", (long long)n);
    GEMHIP_REQUIRE(deg && counts_out, "nbr_plan_host: NULL deg or output");
    for (int64_t i = 0; i < n; ++i) GEMHIP_REQUIRE(deg[i] >= 0 && deg[i] < n, "nbr_plan_host: deg[%lld] = %d outside [0,%lld)", (long long)i, deg[i], (long long)n);
    const int rc = check_pairs("nbr_plan_host", n, m, st, ed);
    if (rc) return rc;
    NbrPlan plan;
    if (!nbr_plan(deg, m, st, ed, plan)) return fail(GEMHIP_E_UNSUPPORTED, "nbr_plan_host: the partial slots of the split pairs reach 2^31");
    counts_out[0] = (int64_t)plan.narrow.size(); counts_out[1] = (int64_t)plan.wide.size(); counts_out[2] = (int64_t)plan.split.size();
    counts_out[3] = plan.slots; counts_out[4] = plan.longest; counts_out[5] = plan.empty;
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_create(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, gemhip_nbr_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "nbr_create: NULL output");
    *out = nullptr;
    int rc = check_graph("nbr_create", n, m, src, dst);
    if (rc) return rc;
    std::unique_ptr<gemhip_nbr> h(new gemhip_nbr);
    h->n = n;
    double t0 = wall_ms();
    std::vector<int64_t> row_ptr;
    std::vector<int32_t> col;
    nbr_build_graph(n, m, src, dst, row_ptr, col, h->deg);
    std::vector<double> w_aa((size_t)n), w_ra((size_t)n);
    nbr_weights(n, h->deg.data(), 0, w_aa.data());
    nbr_weights(n, h->deg.data(), 1, w_ra.data());
    h->nnz = row_ptr[n];
    for (int64_t i = 0; i < n; ++i) h->max_deg = h->deg[i] > h->max_deg ? h->deg[i] : h->max_deg;
    h->ms[0] = wall_ms() - t0;
    t0 = wall_ms();
    GEMHIP_CHECK(h->row_ptr.upload(row_ptr.data(), (size_t)n + 1));
    GEMHIP_CHECK(h->col.upload(col.data(), col.size()));
    GEMHIP_CHECK(h->d_deg.upload(h->deg.data(), (size_t)n));
    GEMHIP_CHECK(h->w_aa.upload(w_aa.data(), (size_t)n));
    GEMHIP_CHECK(h->w_ra.upload(w_ra.data(), (size_t)n));
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->ms[1] = wall_ms() - t0;
    *out = h.release();
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_destroy(gemhip_nbr_t h)
{
    delete h;
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_degrees(gemhip_nbr_t h, int32_t *deg_out)
{
    GEMHIP_REQUIRE(h && deg_out, "nbr_degrees: NULL");
    GEMHIP_CHECK(hipMemcpy(deg_out, h->d_deg, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_weights(gemhip_nbr_t h, int32_t which, double *w_out)
{
    GEMHIP_REQUIRE(h && w_out, "nbr_weights: NULL");
    GEMHIP_REQUIRE(which == 0 || which == 1, "nbr_weights: table %d (0 Adamic-Adar, 1 resource allocation)", which);
    GEMHIP_CHECK(hipMemcpy(w_out, which == 0 ? h->w_aa.get() : h->w_ra.get(), (size_t)h->n * sizeof(double), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_scores(gemhip_nbr_t h, int64_t m, const int32_t *st, const int32_t *ed, int32_t mask, int32_t *cn_out, double *jaccard_out,
                                 double *aa_out, double *ra_out, double *pa_out)
{
    GEMHIP_REQUIRE(h != nullptr, "nbr_scores: NULL handle");
    const int rc = check_pairs("nbr_scores", h->n, m, st, ed);
    if (rc) return rc;
    GEMHIP_REQUIRE(mask >= 1 && mask <= NBR_ALL, "nbr_scores: mask %d outside [1,%d] (1 cn, 2 jaccard, 4 aa, 8 ra, 16 pa)", mask, (int)NBR_ALL);
    GEMHIP_REQUIRE((!(mask & NBR_CN) || cn_out) && (!(mask & NBR_JACCARD) || jaccard_out) && (!(mask & NBR_AA) || aa_out) && (!(mask & NBR_RA) || ra_out) &&
                       (!(mask & NBR_PA) || pa_out), "nbr_scores: NULL output for a score in the mask %d", mask);
    double t0 = wall_ms();
    NbrPlan plan;
    if (!nbr_plan(h->deg.data(), m, st, ed, plan)) return fail(GEMHIP_E_UNSUPPORTED, "nbr_scores: the partial slots of the split pairs reach 2^31");
    h->ms[2] = wall_ms() - t0;
    const int64_t n_narrow = (int64_t)plan.narrow.size(), n_wide = (int64_t)plan.wide.size(), n_split = (int64_t)plan.split.size();
    h->last[0] = n_narrow; h->last[1] = n_wide; h->last[2] = n_split; h->last[3] = plan.slots; h->last[4] = plan.longest; h->last[5] = m;

    t0 = wall_ms();
    GEMHIP_CHECK(h->st.upload(st, (size_t)m));
    GEMHIP_CHECK(h->ed.upload(ed, (size_t)m));
    GEMHIP_CHECK(h->narrow.upload(plan.narrow.data(), plan.narrow.size()));
    GEMHIP_CHECK(h->wide.upload(plan.wide.data(), plan.wide.size()));
    GEMHIP_CHECK(h->split.upload(plan.split.data(), plan.split.size()));
    GEMHIP_CHECK(h->cn.reserve((size_t)m));
    GEMHIP_CHECK(h->jac.reserve((size_t)m));
    GEMHIP_CHECK(h->aa.reserve((size_t)m));
    GEMHIP_CHECK(h->ra.reserve((size_t)m));
    GEMHIP_CHECK(h->pa.reserve((size_t)m));
    GEMHIP_CHECK(h->part_cn.reserve((size_t)plan.slots));
    GEMHIP_CHECK(h->part_aa.reserve((size_t)plan.slots));
    GEMHIP_CHECK(h->part_ra.reserve((size_t)plan.slots));
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->ms[3] = wall_ms() - t0;

    GEMHIP_CHECK(start(h->watch));
    GEMHIP_CHECK(hipMemsetAsync(h->cn, 0, (size_t)m * sizeof(int32_t), 0));          // a pair without an item: all five scores are zero
    for (double *p : {h->jac.get(), h->aa.get(), h->ra.get(), h->pa.get()}) GEMHIP_CHECK(hipMemsetAsync(p, 0, (size_t)m * sizeof(double), 0));
    if (n_narrow) {
        hipLaunchKernelGGL(nbr_score_kernel<NBR_LANES>, dim3(nbr_grid(n_narrow, (WAVE / NBR_LANES) * (NBR_THREADS / WAVE))), dim3(NBR_THREADS), 0, 0, h->row_ptr.get(),
                           h->col.get(), h->d_deg.get(), h->w_aa.get(), h->w_ra.get(), h->st.get(), h->ed.get(), h->narrow.get(), n_narrow, h->cn.get(), h->jac.get(),
                           h->aa.get(), h->ra.get(), h->pa.get(), h->part_cn.get(), h->part_aa.get(), h->part_ra.get());
        GEMHIP_CHECK(hipGetLastError());
    }
    if (n_wide) {
        hipLaunchKernelGGL(nbr_score_kernel<WAVE>, dim3(nbr_grid(n_wide, NBR_THREADS / WAVE)), dim3(NBR_THREADS), 0, 0, h->row_ptr.get(), h->col.get(), h->d_deg.get(),
                           h->w_aa.get(), h->w_ra.get(), h->st.get(), h->ed.get(), h->wide.get(), n_wide, h->cn.get(), h->jac.get(), h->aa.get(), h->ra.get(),
                           h->pa.get(), h->part_cn.get(), h->part_aa.get(), h->part_ra.get());
        GEMHIP_CHECK(hipGetLastError());
    }
    if (n_split) {
        hipLaunchKernelGGL(nbr_finish_kernel, dim3(nbr_grid(n_split, NBR_THREADS)), dim3(NBR_THREADS), 0, 0, h->d_deg.get(), h->st.get(), h->ed.get(), h->split.get(),
                           n_split, h->part_cn.get(), h->part_aa.get(), h->part_ra.get(), h->cn.get(), h->jac.get(), h->aa.get(), h->ra.get(), h->pa.get());
        GEMHIP_CHECK(hipGetLastError());
    }
    GEMHIP_CHECK(stop(h->watch, &h->ms[4]));

    t0 = wall_ms();
    if (mask & NBR_CN) GEMHIP_CHECK(hipMemcpy(cn_out, h->cn, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (mask & NBR_JACCARD) GEMHIP_CHECK(hipMemcpy(jaccard_out, h->jac, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (mask & NBR_AA) GEMHIP_CHECK(hipMemcpy(aa_out, h->aa, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (mask & NBR_RA) GEMHIP_CHECK(hipMemcpy(ra_out, h->ra, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    if (mask & NBR_PA) GEMHIP_CHECK(hipMemcpy(pa_out, h->pa, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
    h->ms[5] = wall_ms() - t0;
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_last_ms(gemhip_nbr_t h, double *out)
{
    GEMHIP_REQUIRE(h && out, "nbr_last_ms: NULL");
    for (int q = 0; q < 6; ++q) out[q] = h->ms[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_nbr_info(gemhip_nbr_t h, int64_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "nbr_info: NULL output");
    out[0] = h ? h->n : 0; out[1] = h ? h->nnz : 0; out[2] = h ? h->max_deg : 0;
    out[3] = NBR_LANES; out[4] = NBR_NARROW; out[5] = NBR_CHUNK;
    for (int q = 0; q < 6; ++q) out[6 + q] = h ? h->last[q] : 0;
    return GEMHIP_OK;
}
