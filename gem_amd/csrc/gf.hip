// gf.hip -- Graph Factorization edge-SGD for MI355X (gfx950).
//
// Replaces gem/embedding/gf.py:93-100 (Python hot loop) and
// gem/c_src/gf.cpp:152-164 (the same loop in the `gf` executable).
//
// Reference semantics (kept exactly):
//   for sweep in range(max_iter):
//     for (i, j, w) in graph.edges():          # grouped by source i, in node-insertion order
//       if j <= i: continue
//       X[i] -= eta * (regu * X[i] - (w - X[i].X[j]) * X[j])     # only row i is written
//
// Device schedule.  Because only the SOURCE row is written and only edges with
// j > i fire, one wavefront can own row i for a whole sweep: X_i lives in
// registers (d=128 -> one float2 per lane), every neighbour row X_j is ONE
// coalesced 4*d-byte read, the dot product is a DPP/readlane wave reduction and
// there are no atomics and no write conflicts.  The sequential (Gauss-Seidel)
// order of the reference is reproduced with two copies of the table:
//   * a row i that the reference visits BEFORE row j reads X_old[j]  (j not yet updated),
//   * a row i visited AFTER row j (j earlier in graph.nodes order but j > i) reads
//     X_new[j]; such rows are placed in a later LEVEL (kernel launch) than j.
// With nodes inserted in ascending id order (every synthetic benchmark graph)
// all rows are level 0 and a sweep is a single launch.  The result differs from
// the fp32 CPU loop only by the summation order inside the dot product.
//
// HBM traffic per sweep (algorithmic, d=128): 512 B read + 512 B write per active
// row, 512 B gather + 8 B (col,w) per update.
//
// The host planning (which edge orders this can represent, levels, hub rows, the unit schedule of any other order) is plain C++ in gf_plan.hip.
#include "common.hpp"
#include "gf_plan.hpp"
#include <hip/hip_cooperative_groups.h>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include <cmath>

using namespace gemhip;

namespace { struct gf_launchers; }

struct gemhip_gf_plan {
    int64_t n = 0, d = 0, nrows = 0, nupd = 0;
    int device = 0;
    const gf_launchers *fn = nullptr; // the kernels instantiated for d (gf_launchers_for)
    std::vector<int64_t> level_off;   // rows of level L are [level_off[L], level_off[L+1])
    std::vector<int64_t> level_hubs;  // ... of which the first level_hubs[L] are hub rows (gf_hub_kernel)
    std::vector<int64_t> level_maxlen;  // longest non-hub row of the level, in firing edges (the rows-per-wavefront rule looks at it)
    hipStream_t hub_stream = nullptr; hipEvent_t hub_fork = nullptr, hub_join = nullptr;
    DevBuf<int32_t> d_rows;           // row ids in processing order (sorted by level, then reference order)
    DevBuf<int64_t> d_ptr;            // CSR offsets over d_rows
    DevBuf<uint32_t> d_col;           // neighbour id | (1u<<31 if that neighbour is read from X_new)
    DevBuf<float> d_w;
    float *X[2] = {nullptr, nullptr};   // the two tables the kernels ping-pong between: X_own's blocks, or the caller's (gemhip_gf_plan_bind)
    DevBuf<float> X_own[2];             // empty while the tables are borrowed
    int cur = 0;                      // X[cur] holds the latest table
    int rows_per_wave = 0;            // 0 = auto (gf_rows_per_wave), else forced (gemhip_gf_plan_set_rows_per_wave: tests, A/B)
    // sweeps per cooperative launch (gf_sweeps_coop_kernel): 0 = off (one launch per sweep and level), k > 1 = up to k sweeps per launch on single-level
    // plans without hub rows; fused_grid caps the resident grid (0 = all the occupancy allows).  GEMHIP_GF_FUSED_SWEEPS / _GRID, gemhip_gf_plan_set_fused_sweeps
    int fused_sweeps = getenv("GEMHIP_GF_FUSED_SWEEPS") ? atoi(getenv("GEMHIP_GF_FUSED_SWEEPS")) : 0;
    int fused_grid = getenv("GEMHIP_GF_FUSED_GRID") ? atoi(getenv("GEMHIP_GF_FUSED_GRID")) : 0;
    // Non-temporal hints of the sweep kernels (GEMHIP_GF_NT_STORE, read per plan; -1 = auto).  bit 1 (value 2): the load of a wave's OWN row -- with rows
    // visited in ascending order it is the row's last use of the sweep (only lower rows gather it, and they ran before), and at SBM 1M/10M an XCD's 4 MB
    // of L2 cannot even hold the 5 MB neighbour set the gathers hit in: marking the own-row stream evict-first took a sweep from 548 to 515 us
    // (profiles/r04_ab_gf_nt.jsonl); bit 0 (value 1): the row stores (measured: no effect); bit 2 (value 4): the (col, w) / row-id / offset streams.
    // Auto: 2 on the K-rows-per-wavefront kernel (the big levels), 0 on the one-row kernel (small, L2-resident levels, where nothing needs evicting).
    // A hint only: results are bit-identical either way.
    int nt_store = getenv("GEMHIP_GF_NT_STORE") ? atoi(getenv("GEMHIP_GF_NT_STORE")) : -1;
    // 1: hub rows run gf_hub_block_kernel (blocks of B edges through a Gram matrix) instead of gf_hub_kernel -- opt-in, within the oracle tolerance but not
    // bit-identical to the row kernels (GEMHIP_GF_HUB_BLOCK=1 read per plan, gemhip_gf_plan_set_hub_block)
    int hub_block = getenv("GEMHIP_GF_HUB_BLOCK") && atoi(getenv("GEMHIP_GF_HUB_BLOCK")) == 1 ? 1 : 0;
    // Unit schedule (gemhip_gf_plan_create_any_order on a list the row schedule cannot represent): the same arrays, read differently (GfHostPlan);
    // nrows counts units.
    bool units = false;
    DevBuf<int64_t> d_level_off;      // level_off on the device (gf_units_fused_kernel walks it)
    std::vector<GfSeg> segs;          // the launches of one sweep (gf_units_segments; gemhip_gf_plan_set_fused_levels recomputes them)
};

namespace {

constexpr int GF_BLOCK = 256;              // 4 waves, one row per wave
constexpr int GF_WAVES = GF_BLOCK / WAVE;
constexpr int GF_PREFETCH = 4;             // neighbour rows in flight per wave
constexpr int GF_HUB_EDGES = 1024;         // rows with at least this many firing edges get a workgroup (gf_hub_kernel)
constexpr int GF_PREFETCH_DEEP = 16;       // ... on full 64-edge chunks of long (hub) rows, divided by the registers a row needs

template <int VEC> struct vec_t;
template <> struct vec_t<1> { using type = float; };
template <> struct vec_t<2> { using type = float2; };

template <int VEC>
__device__ __forceinline__ void load_row(const float *__restrict__ p, int d, int lane, int c, float (&v)[VEC])
{
    const int idx = (c * WAVE + lane) * VEC;
    if constexpr (VEC == 2) {
        if (idx < d) { const float2 t = *reinterpret_cast<const float2 *>(p + idx); v[0] = t.x; v[1] = t.y; }
        else { v[0] = 0.f; v[1] = 0.f; }
    } else {
        v[0] = idx < d ? p[idx] : 0.f;
    }
}

// a wave's OWN row: with rows visited in ascending order its last use of the sweep (only lower rows gather it, and they ran before) -- bit 2 of the
// plan's nt_store asks for the non-temporal hint on this load as well
template <int VEC>
__device__ __forceinline__ void load_own_row(const float *__restrict__ p, int d, int lane, int c, float (&v)[VEC], int nt)
{
    const int idx = (c * WAVE + lane) * VEC;
    if (!(nt & 2)) { load_row<VEC>(p, d, lane, c, v); return; }
    if constexpr (VEC == 2) {
        typedef float gf_f2 __attribute__((ext_vector_type(2)));
        if (idx < d) { const gf_f2 t = __builtin_nontemporal_load(reinterpret_cast<const gf_f2 *>(p + idx)); v[0] = t.x; v[1] = t.y; }
        else { v[0] = 0.f; v[1] = 0.f; }
    } else {
        v[0] = idx < d ? __builtin_nontemporal_load(p + idx) : 0.f;
    }
}

template <int VEC, int NV>
__device__ __forceinline__ void store_row(float *po, int d, int lane, const float (&xi)[NV][VEC], int nt)
{
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const int idx = (c * WAVE + lane) * VEC;
        if (idx < d) {
            if constexpr (VEC == 2) {
                typedef float gf_f2 __attribute__((ext_vector_type(2)));
                gf_f2 v; v.x = xi[c][0]; v.y = xi[c][1];
                if (nt & 1) __builtin_nontemporal_store(v, reinterpret_cast<gf_f2 *>(po + idx));
                else *reinterpret_cast<gf_f2 *>(po + idx) = v;
            } else {
                if (nt & 1) __builtin_nontemporal_store(xi[c][0], po + idx);
                else po[idx] = xi[c][0];
            }
        }
    }
}

// One edge update X_i -= eta * (regu * X_i - (w_ij - X_i.X_j) * X_j)  (gf.cpp:162-163).  Shared by the wave-per-row kernel and the hub
// kernel: the same expressions are contracted the same way, so both produce bit-identical rows.
template <int VEC, int NV>
__device__ __forceinline__ void gf_apply_edge(float (&xi)[NV][VEC], const float (&xj)[NV][VEC], float wij, float eta, float regu)
{
    // explicit fused / rounded operations: the compiler may not choose between mul+add and fma (or packed forms) differently per kernel
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int v = 0; v < VEC; ++v) part = fmaf(xi[q][v], xj[q][v], part);
    const float coef = wij - wave_sum(part);        // (w_ij - X_i.X_j)
#pragma unroll
    for (int q = 0; q < NV; ++q)
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const float t = fmaf(-coef, xj[q][v], __fmul_rn(regu, xi[q][v]));     // regu * X_i - coef * X_j
            xi[q][v] = fmaf(-eta, t, xi[q][v]);
        }
}

// Apply the updates of up to 64 edges of one row (columns/weights in lane registers cj/wj), U neighbour rows in flight.
// (A rolling window that re-issues a load right after each consumed row measured 6-15 % SLOWER than these plain batches; U = 2 / 4 / 6 / 8 at SBM 1M/10M:
// 0.648 / 0.598 / 0.598 / 0.610 ms per sweep.)
template <int VEC, int NV, int U>
__device__ __forceinline__ void gf_chunk(float (&xi)[NV][VEC], uint32_t cj, float wj, int cnt, const float *Xold, const float *Xnew, int d, int lane,
                                         float eta, float regu)
{
    for (int k = 0; k < cnt; k += U) {
        float xj[U][NV][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = (k + u) < cnt ? (k + u) : (cnt - 1);
            const uint32_t c = bcast_lane(cj, kk);
            const float *pj = ((c >> 31) ? Xnew : Xold) + (int64_t)(c & 0x7fffffffu) * d;
#pragma unroll
            for (int q = 0; q < NV; ++q) load_row<VEC>(pj, d, lane, q, xj[u][q]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (k + u < cnt) gf_apply_edge<VEC, NV>(xi, xj[u], bcast_lane(wj, k + u), eta, regu);
    }
}

// neighbour rows in flight on FULL 64-edge chunks.  Hub rows (power-law graphs) are one long dependent chain of updates: only memory latency can be
// hidden, so full chunks keep GF_PREFETCH_DEEP / NV (at least GF_PREFETCH) neighbour rows in flight instead of GF_PREFETCH
template <int NV> constexpr int GF_DEEP = (GF_PREFETCH_DEEP / NV) >= GF_PREFETCH ? (GF_PREFETCH_DEEP / NV) : GF_PREFETCH;

// one row's chunk of `cnt` edges whose (col, w) lane `k` holds for edge k
template <int VEC, int NV>
__device__ __forceinline__ void gf_apply_chunk(float (&xi)[NV][VEC], uint32_t cj, float wj, int cnt, const float *Xold, const float *Xnew, int d, int lane,
                                               float eta, float regu)
{
    if (cnt == WAVE) gf_chunk<VEC, NV, GF_DEEP<NV>>(xi, cj, wj, cnt, Xold, Xnew, d, lane, eta, regu);
    else gf_chunk<VEC, NV, GF_PREFETCH>(xi, cj, wj, cnt, Xold, Xnew, d, lane, eta, regu);
}

// a plan stream (col, w, row ids, offsets), read once per sweep: bit 2 of the plan's nt_store asks for the non-temporal hint
template <typename T> __device__ __forceinline__ T gf_ld_stream(const T *p, int nt) { return (nt & 4) ? __builtin_nontemporal_load(p) : *p; }

// THE row body of every wave-per-row kernel: the edges [e, e1) of one row applied to xi in edge order, 64 at a time
template <int VEC, int NV>
__device__ __forceinline__ void gf_row_edges(float (&xi)[NV][VEC], int64_t e, int64_t e1, const uint32_t *__restrict__ col, const float *__restrict__ w,
                                             const float *Xold, const float *Xnew, int d, int lane, float eta, float regu, int nt)
{
    for (; e < e1; e += WAVE) {
        const int cnt = (int)((e1 - e) < (int64_t)WAVE ? (e1 - e) : (int64_t)WAVE);
        // coalesced read of up to 64 (col, w) pairs of this row; broadcast later with v_readlane
        const uint32_t cj = lane < cnt ? gf_ld_stream(col + e + lane, nt) : 0u;
        const float wj = lane < cnt ? gf_ld_stream(w + e + lane, nt) : 0.f;
        gf_apply_chunk<VEC, NV>(xi, cj, wj, cnt, Xold, Xnew, d, lane, eta, regu);
    }
}

// One sweep over the rows of one level.  One wavefront per row.
template <int VEC, int NV>
__global__ __launch_bounds__(GF_BLOCK) void gf_sweep_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                            const uint32_t *__restrict__ col, const float *__restrict__ w,
                                                            const float *Xold, float *Xnew, int64_t row0, int64_t nrows, int d,
                                                            float eta, float regu, int nt)
{
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t slot = xcd_contiguous_block(blockIdx.x, gridDim.x) * GF_WAVES + wave;
    if (slot >= nrows) return;
    const int64_t r = row0 + slot;
    const int32_t i = rows[r];
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];

    float xi[NV][VEC];
    const float *pi = Xold + (int64_t)i * d;
#pragma unroll
    for (int c = 0; c < NV; ++c) load_own_row<VEC>(pi, d, lane, c, xi[c], nt);
    gf_row_edges<VEC, NV>(xi, e0, e1, col, w, Xold, Xnew, d, lane, eta, regu, 0);
    store_row<VEC, NV>(Xnew + (int64_t)i * d, d, lane, xi, nt);
}

// Several sweeps in ONE launch (round 5; experiment behind gemhip_gf_plan_set_fused_sweeps / GEMHIP_GF_FUSED_SWEEPS).  At SBM 10k/100k (BASELINE configs[1])
// a sweep is a ~5 us kernel and 1000 of them cost 9 us each: the loop is launch-bound.  This kernel keeps the grid resident (cooperative launch: every
// workgroup co-resident by construction) and separates the sweeps with cooperative_groups' grid barrier, which carries the agent-scope release / acquire
// that makes the rows one XCD wrote visible to the other seven (L2 write-back + invalidate: what a kernel boundary does).  Same row body as
// gf_sweep_kernel, same edge order: bit-identical tables.  Single-level plans without hub rows only (every benchmark graph).
template <int VEC, int NV>
__global__ __launch_bounds__(GF_BLOCK) void gf_sweeps_coop_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                                  const uint32_t *__restrict__ col, const float *__restrict__ w, float *X0, float *X1,
                                                                  int64_t nrows, int d, float eta, float regu, int nsweeps)
{
    cooperative_groups::grid_group grid = cooperative_groups::this_grid();
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t nslots = (int64_t)gridDim.x * GF_WAVES;
    const int64_t first = xcd_contiguous_block(blockIdx.x, gridDim.x) * GF_WAVES + wave;
    for (int s = 0; s < nsweeps; ++s) {
        const float *Xold = (s & 1) ? X1 : X0;
        float *Xnew = (s & 1) ? X0 : X1;
        for (int64_t r = first; r < nrows; r += nslots) {
            const int32_t i = rows[r];
            const int64_t e0 = ptr[r], e1 = ptr[r + 1];
            float xi[NV][VEC];
            const float *pi = Xold + (int64_t)i * d;
#pragma unroll
            for (int c = 0; c < NV; ++c) load_row<VEC>(pi, d, lane, c, xi[c]);
            gf_row_edges<VEC, NV>(xi, e0, e1, col, w, Xold, Xnew, d, lane, eta, regu, 0);
            store_row<VEC, NV>(Xnew + (int64_t)i * d, d, lane, xi, 0);
        }
        grid.sync();
    }
}

template <int VEC, int NV>
int launch_coop(const gemhip_gf_plan *p, float *X0, float *X1, float eta, float regu, int nsweeps, hipStream_t s)
{
    // resident workgroups of this instantiation on this device: queried once (both calls are millisecond-scale host work, and the fused path launches
    // once per `fused_sweeps` sweeps -- ADVICE r5).  The kernel reads Xold only: the caller takes this path for single-level plans alone (nlevels == 1 at
    // the launch site), and those never set the "read Xnew" column bit (bit 31).
    static int64_t resident = 0;
    if (resident == 0) {
        int per_cu = 0, dev = 0;
        hipDeviceProp_t prop;
        GEMHIP_CHECK(hipGetDevice(&dev));
        GEMHIP_CHECK(hipGetDeviceProperties(&prop, dev));
        GEMHIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gf_sweeps_coop_kernel<VEC, NV>, GF_BLOCK, 0));
        resident = (int64_t)per_cu * prop.multiProcessorCount;
    }
    int64_t grid = std::min<int64_t>(resident, (p->nrows + GF_WAVES - 1) / GF_WAVES);
    grid = std::max<int64_t>(NUM_XCD, grid / NUM_XCD * NUM_XCD);              // a multiple of 8: the XCD-contiguous map covers every slot
    if (p->fused_grid > 0) grid = std::max<int64_t>(NUM_XCD, std::min<int64_t>(grid, (int64_t)p->fused_grid / NUM_XCD * NUM_XCD));
    const int32_t *rows = p->d_rows; const int64_t *ptr = p->d_ptr; const uint32_t *col = p->d_col; const float *w = p->d_w;
    int64_t nrows = p->nrows; int d = (int)p->d;
    void *args[] = {(void *)&rows, (void *)&ptr, (void *)&col, (void *)&w, (void *)&X0, (void *)&X1, (void *)&nrows, (void *)&d, (void *)&eta, (void *)&regu, (void *)&nsweeps};
    GEMHIP_CHECK(hipLaunchCooperativeKernel((const void *)gf_sweeps_coop_kernel<VEC, NV>, dim3((unsigned)grid), dim3(GF_BLOCK), args, 0, s));
    return GEMHIP_OK;
}

// The same sweep with K consecutive rows per wavefront (large levels; round 4).  A wave that owns ONE row spends its life in a chain of dependent
// round trips -- row id and edge offsets, then (col, w) and X_i, then the neighbour rows, then the store -- and only the third moves data: at SBM
// 1M/10M the kernel reached 3.3 TB/s of real traffic (0.53 of a copy).  Here lane k of a wave fetches the id and the offsets of its k-th row in ONE
// load, and while row k is trained the (col, w) chunk and X_i of row k+1 are already in flight, so the only exposed latency per row is the gather of
// its neighbour rows.  Same gf_apply_edge, same edge order inside a row: bit-identical to gf_sweep_kernel (rows of one level are independent).
template <int VEC, int NV>
__global__ __launch_bounds__(GF_BLOCK) void gf_sweep_rows_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                                 const uint32_t *__restrict__ col, const float *__restrict__ w,
                                                                 const float *Xold, float *Xnew, int64_t row0, int64_t nrows, int d,
                                                                 float eta, float regu, int K, int nt)
{
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    // K CONSECUTIVE rows.  (Measured and dropped, round 4: striping a wavefront's rows 512 / 1024 / 2048 apart inside super-blocks, so that the
    // wavefronts resident on an XCD work in one band of rows at a time -- 560 / 567 / 567 us against 564: the L2 misses of the neighbour gathers are
    // capacity misses of a 5 MB block in 4 MB of L2, not a matter of which rows run together.)
    const int64_t first = (xcd_contiguous_block(blockIdx.x, gridDim.x) * GF_WAVES + wave) * K;
    if (first >= nrows) return;
    const int nk = (int)((nrows - first) < (int64_t)K ? (nrows - first) : (int64_t)K);
    int32_t rv = 0; int64_t pa = 0, pb = 0;
    if (lane < nk) {
        rv = gf_ld_stream(rows + row0 + first + lane, nt);
        pa = gf_ld_stream(ptr + row0 + first + lane, nt); pb = gf_ld_stream(ptr + row0 + first + lane + 1, nt);
    }
    auto lane64 = [&](int64_t v, int k) -> int64_t {
        const uint32_t lo = bcast_lane((uint32_t)v, k), hi = bcast_lane((uint32_t)((uint64_t)v >> 32), k);
        return (int64_t)(((uint64_t)hi << 32) | lo);
    };
    int32_t i_n; int64_t e0_n, e1_n; int cnt_n; uint32_t cj_n; float wj_n;
    float xi_n[NV][VEC];
    auto fetch = [&](int k) {                            // row k of this wavefront: its id and offsets, then its first (col, w) chunk and X_i
        i_n = bcast_lane(rv, k);
        e0_n = lane64(pa, k); e1_n = lane64(pb, k);
        cnt_n = (int)((e1_n - e0_n) < (int64_t)WAVE ? (e1_n - e0_n) : (int64_t)WAVE);
        cj_n = lane < cnt_n ? gf_ld_stream(col + e0_n + lane, nt) : 0u;
        wj_n = lane < cnt_n ? gf_ld_stream(w + e0_n + lane, nt) : 0.f;
#pragma unroll
        for (int c = 0; c < NV; ++c) load_own_row<VEC>(Xold + (int64_t)i_n * d, d, lane, c, xi_n[c], nt);
    };
    fetch(0);
    for (int k = 0; k < nk; ++k) {
        const int32_t i = i_n;
        const int64_t e0 = e0_n, e1 = e1_n;
        const int cnt0 = cnt_n;
        const uint32_t cj0 = cj_n;
        const float wj0 = wj_n;
        float xi[NV][VEC];
#pragma unroll
        for (int c = 0; c < NV; ++c)
#pragma unroll
            for (int v = 0; v < VEC; ++v) xi[c][v] = xi_n[c][v];
        if (k + 1 < nk) fetch(k + 1);                    // the next row's inputs travel while this row is trained
        if (cnt0 > 0) gf_apply_chunk<VEC, NV>(xi, cj0, wj0, cnt0, Xold, Xnew, d, lane, eta, regu);      // the chunk that travelled with the row before
        gf_row_edges<VEC, NV>(xi, e0 + WAVE, e1, col, w, Xold, Xnew, d, lane, eta, regu, nt);
        store_row<VEC, NV>(Xnew + (int64_t)i * d, d, lane, xi, nt);
    }
}

// rows per wavefront of the sweep launch over `nrows` rows of level l (gf_level_rows_per_wave; at most GEMHIP_GF_ROWS_PER_WAVE, default 8, read once)
int gf_rows_per_wave(const gemhip_gf_plan *p, size_t l, int64_t nrows)
{
    static const int kmax = getenv("GEMHIP_GF_ROWS_PER_WAVE") ? std::max(1, std::min(64, atoi(getenv("GEMHIP_GF_ROWS_PER_WAVE")))) : 8;
    return gf_level_rows_per_wave(p->rows_per_wave, l < p->level_maxlen.size() ? p->level_maxlen[l] : 0, nrows, kmax);
}

// workgroups of GF_WAVES wavefronts for `waves` of them, rounded up to a multiple of 8 so the XCD-contiguous map covers every slot
dim3 gf_grid(int64_t waves) { return dim3((unsigned)(((waves + GF_WAVES - 1) / GF_WAVES + NUM_XCD - 1) / NUM_XCD * NUM_XCD)); }

// the rows [row0, row0 + nrows) of level l
template <int VEC, int NV>
void launch_sweep(const gemhip_gf_plan *p, int l, int64_t row0, int64_t nrows, const float *Xold, float *Xnew, float eta, float regu, hipStream_t s)
{
    const int K = gf_rows_per_wave(p, (size_t)l, nrows);
    if (K > 1)
        hipLaunchKernelGGL((gf_sweep_rows_kernel<VEC, NV>), gf_grid((nrows + K - 1) / K), dim3(GF_BLOCK), 0, s, p->d_rows, p->d_ptr, p->d_col,
                           p->d_w, Xold, Xnew, row0, nrows, (int)p->d, eta, regu, K, p->nt_store < 0 ? 2 : p->nt_store);
    else
        hipLaunchKernelGGL((gf_sweep_kernel<VEC, NV>), gf_grid(nrows), dim3(GF_BLOCK), 0, s, p->d_rows, p->d_ptr, p->d_col,
                           p->d_w, Xold, Xnew, row0, nrows, (int)p->d, eta, regu, p->nt_store < 0 ? 0 : p->nt_store);
}

// Hub rows (power-law graphs).  The updates of one row are one dependent chain (exact Gauss-Seidel): a wave that also fetches its
// neighbour rows pays a memory latency per batch on top of the chain (130 ns per update measured).  Here a row with >= GF_HUB_EDGES firing
// edges gets a whole workgroup: wavefronts 1-NP stream the neighbour rows (and weights) of successive batches through an LDS ring, wave 0
// does nothing but apply them, in edge order, with the very same gf_apply_edge -- bit-identical to the wave-per-row kernel.
typedef __attribute__((address_space(3))) volatile int32_t gf_lds_vi32;
__device__ __forceinline__ int32_t gf_flag_ld(const int32_t *p) { return *(gf_lds_vi32 *)p; }
__device__ __forceinline__ void gf_flag_st(int32_t *p, int32_t v) { *(gf_lds_vi32 *)p = v; }

template <int VEC, int NV, int NP>
__global__ __launch_bounds__((NP + 1) * 64) void gf_hub_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                     const uint32_t *__restrict__ col, const float *__restrict__ w, const float *Xold,
                                                     float *Xnew, int64_t row0, int d, float eta, float regu)
{
    constexpr int RW = NV * VEC * WAVE;              // floats of one staged row
    constexpr int B = NV >= 8 ? 2 : 16 / NV;         // edges per batch
    constexpr int NBATCH = NP + 1;                   // ring depth in batches: one per producer wavefront + the one being consumed (8 KB of rows each)
    constexpr int G = B >= 4 ? 4 : B;                // rows the consumer moves LDS -> registers at a time
    __shared__ __attribute__((aligned(16))) float ring[NBATCH * B * RW];
    __shared__ float wring[NBATCH * 16];
    __shared__ int32_t ready[NBATCH];
    __shared__ int32_t done;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int64_t r = row0 + blockIdx.x;
    const int32_t i = rows[r];
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    const int nb = (int)((e1 - e0 + B - 1) / B);
    if (threadIdx.x == 0) done = 0;
    if (threadIdx.x < NBATCH) ready[threadIdx.x] = 0;
    __syncthreads();
    if (wave == 0) {
        float xi[NV][VEC];
        const float *pi = Xold + (int64_t)i * d;
#pragma unroll
        for (int c = 0; c < NV; ++c) load_row<VEC>(pi, d, lane, c, xi[c]);
        auto lds_row = [&](const float *row, float (&v)[NV][VEC]) {
#pragma unroll
            for (int q = 0; q < NV; ++q)
#pragma unroll
                for (int k = 0; k < VEC; ++k) v[q][k] = row[(q * WAVE + lane) * VEC + k];
        };
        for (int t = 0; t < nb; ++t) {
            const int sb = t % NBATCH;
            while (gf_flag_ld(&ready[sb]) != t + 1) __builtin_amdgcn_s_sleep(0);
            asm volatile("" ::: "memory");
            const int cnt = (int)((e1 - (e0 + (int64_t)t * B)) < B ? (e1 - (e0 + (int64_t)t * B)) : B);
            const float wv = wring[sb * 16 + (lane & 15)];
            const float *base = ring + (size_t)sb * B * RW;
            float buf[2][G][NV][VEC];
#pragma unroll
            for (int u = 0; u < G; ++u) lds_row(base + (size_t)u * RW, buf[0][u]);
#pragma unroll
            for (int g = 0; g < B / G; ++g) {
                if (g + 1 < B / G) {
#pragma unroll
                    for (int u = 0; u < G; ++u) lds_row(base + (size_t)((g + 1) * G + u) * RW, buf[(g + 1) & 1][u]);
                }
#pragma unroll
                for (int u = 0; u < G; ++u)
                    if (g * G + u < cnt) gf_apply_edge<VEC, NV>(xi, buf[g & 1][u], bcast_lane(wv, g * G + u), eta, regu);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) gf_flag_st(&done, t + 1);
        }
        store_row<VEC, NV>(Xnew + (int64_t)i * d, d, lane, xi, 0);
    } else {
        for (int t = wave - 1; t < nb; t += NP) {
            const int sb = t % NBATCH;
            while (gf_flag_ld(&done) < t - NBATCH + 1) __builtin_amdgcn_s_sleep(1);     // the batch that used this ring segment is consumed
            asm volatile("" ::: "memory");
            const int64_t eb = e0 + (int64_t)t * B;
            const int cnt = (int)((e1 - eb) < B ? (e1 - eb) : B);
            const uint32_t cj = lane < cnt ? col[eb + lane] : 0u;
            const float wj = lane < cnt ? w[eb + lane] : 0.f;
            float xj[B][NV][VEC];
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const int kk = u < cnt ? u : cnt - 1;
                const uint32_t c = bcast_lane(cj, kk);
                const float *pj = ((c >> 31) ? Xnew : Xold) + (int64_t)(c & 0x7fffffffu) * d;
#pragma unroll
                for (int q = 0; q < NV; ++q) load_row<VEC>(pj, d, lane, q, xj[u][q]);
            }
            float *base = ring + (size_t)sb * B * RW;
#pragma unroll
            for (int u = 0; u < B; ++u)
#pragma unroll
                for (int q = 0; q < NV; ++q)
#pragma unroll
                    for (int k = 0; k < VEC; ++k) base[(size_t)u * RW + (q * WAVE + lane) * VEC + k] = xj[u][q][k];
            if (lane < 16) wring[sb * 16 + lane] = wj;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) gf_flag_st(&ready[sb], t + 1);
        }
    }
}

template <int VEC, int NV>
void launch_hub(const gemhip_gf_plan *p, int64_t row0, int64_t nhub, const float *Xold, float *Xnew, float eta, float regu, hipStream_t s)
{
    // producer wavefronts per hub row: the chain's wavefront consumes a neighbour row every ~50 ns, a producer needs two loaded-HBM round
    // trips per batch of 16 while the wave-per-row kernel saturates the memory system next to it (GEMHIP_GF_HUB_PRODUCERS=3|7 for the A/B)
    static const int np = getenv("GEMHIP_GF_HUB_PRODUCERS") ? atoi(getenv("GEMHIP_GF_HUB_PRODUCERS")) : 7;
    if (np >= 7)
        hipLaunchKernelGGL((gf_hub_kernel<VEC, NV, 7>), dim3((unsigned)nhub), dim3(512), 0, s, p->d_rows, p->d_ptr, p->d_col, p->d_w, Xold, Xnew, row0,
                           (int)p->d, eta, regu);
    else
        hipLaunchKernelGGL((gf_hub_kernel<VEC, NV, 3>), dim3((unsigned)nhub), dim3(256), 0, s, p->d_rows, p->d_ptr, p->d_col, p->d_w, Xold, Xnew, row0,
                           (int)p->d, eta, regu);
}

// ---- blocked hub rows (gemhip_gf_plan_set_hub_block; opt-in, NOT bit-identical to the row kernels).  gf_hub_kernel takes the memory latency out of a
// hub row's chain; what remains is the chain: per edge one dot product, a wave reduction, a scalar and an axpy, each waiting for the one before.
// Within one row's pass every neighbour row is constant (only row i is written), so the update is affine in x_i, and B edges (neighbour rows y_t,
// weights w_t, a = 1 - eta * regu) can be applied at once: with G = Y Y^T and p = Y x_0,
//     s_t = w_t - a^(t-1) p_t - eta * sum_{u<t} a^(t-1-u) s_u G_tu,        x_B = a^B x_0 + sum_u (eta * a^(B-u) s_u) y_u.
// The producers stage B neighbour rows in LDS as gf_hub_kernel's do and form G on the matrix units with the fp32-input MFMA (exact fp32); G does
// not depend on x, so it runs ahead of the chain.  The consumer wavefront computes p (lane = row of the block, 64 / B lanes share a row and each
// reads a contiguous piece of it), runs the B-step substitution without any reduction -- lane v keeps r_v = x_t . y_v up to date with
// r_v <- r_v - (eta regu) r_v + eta s_t G_vt, one broadcast and two FMAs per step -- and applies the GEMV.  The powers of a that scale x and the
// coefficients come from gf_hub_decay (evaluated in double, hi + lo where they scale x).  No atomics, one fixed summation order: a row's result
// depends only on its edge list and its inputs, not on the producer count or on timing.
struct GfHubDecay { float hi[GF_HUB_BLOCK_MAX + 1], lo[GF_HUB_BLOCK_MAX + 1]; };
typedef float gf_f32x2 __attribute__((ext_vector_type(2)));
typedef float gf_f32x4 __attribute__((ext_vector_type(4)));
typedef float gf_f32x16 __attribute__((ext_vector_type(16)));

template <int VEC, int NV, int NP> struct gf_hub_block_cfg {
    static constexpr int RW = NV * VEC * WAVE;                 // floats of one staged row
    static constexpr int B = gf_hub_block_of_row_floats(RW);   // edges per block
    // rows are 4 floats apart from a multiple of 64: the 16 lanes of a ds_read_b128 group that read 16 different rows at one column hit 16
    // different 16-byte slots of the 256-byte bank row (the access pattern of p = Y x and of the MFMA operand reads)
    static constexpr int RS = RW + 4;
    static constexpr int NSEG = WAVE / B;                      // lanes per row of the block ...
    static constexpr int L = RW / NSEG;                        // ... each reading this many contiguous floats of it
    static constexpr int STAGE = B * RS + B * B + B;           // floats of one ring stage: the rows, G, the weights
    // stages: what fits 64 KB with the rest of the workgroup's LDS, so that two hub rows share a CU (160 KB) as gf_hub_kernel's do -- on a power-law
    // graph the hub rows together, not only the longest, set the sweep time (1024 rows of 4096 edges: 1.01 ms at one workgroup per CU against 0.66 ms
    // of gf_hub_kernel at two); at least 2, which for the widest rows is one workgroup per CU
    static constexpr int FIT = (64 * 1024 - NSEG * (L + 4) * 4 - 64) / (STAGE * 4);
    static constexpr int NST = FIT > NP ? NP : FIT < 2 ? 2 : FIT;
    static constexpr int PF0 = 64 / (NV * VEC);                // neighbour rows a producer has in flight: 64 registers' worth, 2 .. B
    static constexpr int PF = PF0 > B ? B : PF0 < 2 ? 2 : PF0;
    static_assert(B <= GF_HUB_BLOCK_MAX && B % PF == 0 && L % 4 == 0 && (NST * STAGE + NSEG * (L + 4)) * 4 + 64 <= 160 * 1024, "LDS layout");
};

template <int VEC, int NV, int NP>
__global__ __launch_bounds__((NP + 1) * 64) void gf_hub_block_kernel(const int32_t *__restrict__ rows, const int64_t *__restrict__ ptr,
                                                                     const uint32_t *__restrict__ col, const float *__restrict__ w, const float *Xold,
                                                                     float *Xnew, int64_t row0, int d, float eta, float regu, GfHubDecay dec)
{
    using cfg = gf_hub_block_cfg<VEC, NV, NP>;
    constexpr int B = cfg::B, RS = cfg::RS, L = cfg::L, STAGE = cfg::STAGE, NST = cfg::NST, PF = cfg::PF;
    __shared__ __attribute__((aligned(16))) float ring[NST * STAGE];
    __shared__ __attribute__((aligned(16))) float xs[cfg::NSEG * (L + 4)];        // x_0 of the block, each lane group's piece 4 floats further (banks)
    __shared__ int32_t ready[NST];
    __shared__ int32_t done;
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    const int row = lane % B, seg = lane / B;
    const int64_t r = row0 + blockIdx.x;
    const int32_t i = rows[r];
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    const int nb = __builtin_amdgcn_readfirstlane((int)((e1 - e0 + B - 1) / B));
    if (threadIdx.x == 0) done = 0;
    if (threadIdx.x < NST) ready[threadIdx.x] = 0;
    __syncthreads();
    if (wave == 0) {
        float xi[NV][VEC];
        const float *pi = Xold + (int64_t)i * d;
#pragma unroll
        for (int c = 0; c < NV; ++c) load_row<VEC>(pi, d, lane, c, xi[c]);
        const float el = __fmul_rn(eta, regu);
        const float tab_hi = dec.hi[lane < B ? lane : B], tab_lo = dec.lo[lane < B ? lane : B];       // lane k holds a^k
        const float hi_full = dec.hi[B], lo_full = dec.lo[B], hrev_full = dec.hi[B - 1 - row];
        for (int t = 0; t < nb; ++t) {
            const int sb = t % NST;
            const int64_t left = e1 - (e0 + (int64_t)t * B);
            const int m = __builtin_amdgcn_readfirstlane((int)(left < B ? left : B));
#pragma unroll
            for (int q = 0; q < NV; ++q)
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const int e = (q * WAVE + lane) * VEC + k;
                    xs[e + (e / L) * 4] = xi[q][k];
                }
            while (gf_flag_ld(&ready[sb]) != t + 1) __builtin_amdgcn_s_sleep(0);
            asm volatile("" ::: "memory");
            const float *st = ring + (size_t)sb * STAGE, *Gs = st + B * RS, *ws = Gs + B * B;
            // p = Y x_0: this lane's piece of row `row`, then the pieces of a row added across its lanes (every lane of a row ends with the same sum)
            const gf_f32x4 *yr = reinterpret_cast<const gf_f32x4 *>(st + row * RS + seg * L);
            const gf_f32x4 *xr = reinterpret_cast<const gf_f32x4 *>(xs + seg * (L + 4));
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
            for (int j = 0; j < L / 4; ++j) {
                const gf_f32x4 y = yr[j], x = xr[j];
                a0 = fmaf(y.x, x.x, a0); a1 = fmaf(y.y, x.y, a1); a2 = fmaf(y.z, x.z, a2); a3 = fmaf(y.w, x.w, a3);
            }
            float rv = __fadd_rn(__fadd_rn(a0, a1), __fadd_rn(a2, a3));
#pragma unroll
            for (int o = B; o < WAVE; o <<= 1) rv = __fadd_rn(rv, __shfl_xor(rv, o));
            // the substitution: rv = x_u . y_row while step u runs.  A last partial block runs all B steps too -- its rows past m repeat row m - 1
            // with weight 0, finite work whose coefficients are dropped below
            float g[B];
#pragma unroll
            for (int u = 0; u < B; ++u) g[u] = Gs[u * B + row];                    // G is symmetric: column `row` read as a row, lane-contiguous
            const float ew = __fmul_rn(eta, ws[row]);
            float esm = 0.f;
#pragma unroll
            for (int u = 0; u < B; ++u) {
                // eta s_u = eta (w_u - x_u . y_u): per step the chain is one broadcast and two FMAs, the decay of rv runs beside it
                const float es = fmaf(-eta, bcast_lane(rv, u), bcast_lane(ew, u));
                esm = row == u ? es : esm;
                rv = fmaf(es, g[u], fmaf(-el, rv, rv));
            }
            const int back = m - 1 - row;
            const float hrev = m == B ? hrev_full : __shfl(tab_hi, back > 0 ? back : 0);
            const float cm = row < m ? __fmul_rn(esm, hrev) : 0.f;                 // eta a^(m-1-u) s_u
            const float him = m == B ? hi_full : bcast_lane(tab_hi, m), lom = m == B ? lo_full : bcast_lane(tab_lo, m);
            // x_m = a^m x_0 + sum_u c_u y_u, the small terms summed first
            float acc[NV][VEC];
#pragma unroll
            for (int q = 0; q < NV; ++q)
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc[q][k] = __fmul_rn(lom, xi[q][k]);
#pragma unroll
            for (int u = 0; u < B; ++u) {
                const float cu = bcast_lane(cm, u);
                const float *yu = st + u * RS;
#pragma unroll
                for (int q = 0; q < NV; ++q) {
                    if constexpr (VEC == 2) {
                        const gf_f32x2 y = *reinterpret_cast<const gf_f32x2 *>(yu + (q * WAVE + lane) * 2);
                        acc[q][0] = fmaf(cu, y.x, acc[q][0]); acc[q][1] = fmaf(cu, y.y, acc[q][1]);
                    } else {
                        acc[q][0] = fmaf(cu, yu[q * WAVE + lane], acc[q][0]);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < NV; ++q)
#pragma unroll
                for (int k = 0; k < VEC; ++k) xi[q][k] = fmaf(him, xi[q][k], acc[q][k]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) gf_flag_st(&done, t + 1);
        }
        store_row<VEC, NV>(Xnew + (int64_t)i * d, d, lane, xi, 0);
    } else {
        // A workgroup's wavefronts go to the four SIMDs in turn, so wavefront 4 sits on the chain's SIMD: it stays idle.  (As a producer its MFMAs and
        // LDS reads cost the chain 52 ns per edge against 44.5 ns without it, one 100k-edge row at d = 128; R-MAT-22: 6.19 against 5.88 ms per sweep.)
        constexpr int NPE = NP > 3 ? NP - 1 : NP;
        if (NP > 3 && wave == 4) return;
        const int pid = wave < 4 ? wave - 1 : wave - 2;
        for (int t = pid; t < nb; t += NPE) {
            const int sb = t % NST;
            const int64_t eb = e0 + (int64_t)t * B;
            const int cnt = __builtin_amdgcn_readfirstlane((int)((e1 - eb) < B ? (e1 - eb) : B));
            const uint32_t cj = lane < cnt ? col[eb + lane] : 0u;
            const float wj = lane < cnt ? w[eb + lane] : 0.f;
            float xj[PF][NV][VEC];
            auto fetch = [&](int g0) {                                             // rows g0 .. g0 + PF - 1 of the block; past the end: the last edge's row again
#pragma unroll
                for (int u = 0; u < PF; ++u) {
                    const int kk = (g0 + u) < cnt ? (g0 + u) : cnt - 1;
                    const uint32_t c = bcast_lane(cj, kk);
                    const float *pj = ((c >> 31) ? Xnew : Xold) + (int64_t)(c & 0x7fffffffu) * d;
#pragma unroll
                    for (int q = 0; q < NV; ++q) load_row<VEC>(pj, d, lane, q, xj[u][q]);
                }
            };
            fetch(0);                                                              // travels while the ring stage is still in use
            while (gf_flag_ld(&done) < t - NST + 1) __builtin_amdgcn_s_sleep(1);   // the block that used this ring stage is consumed
            asm volatile("" ::: "memory");
            float *st = ring + (size_t)sb * STAGE, *Gs = st + B * RS;
#pragma unroll
            for (int g0 = 0; g0 < B; g0 += PF) {
#pragma unroll
                for (int u = 0; u < PF; ++u)
#pragma unroll
                    for (int q = 0; q < NV; ++q)
#pragma unroll
                        for (int k = 0; k < VEC; ++k) st[(g0 + u) * RS + (q * WAVE + lane) * VEC + k] = xj[u][q][k];
                if (g0 + PF < B) fetch(g0 + PF);
            }
            if (lane < B) Gs[B * B + lane] = wj;
            // G = Y Y^T on the matrix units.  A lane supplies one element of row `row` per instruction, as the A operand and (G's column = a row of Y) as the
            // B operand alike; WHICH k a lane group supplies is free as long as both operands agree, so each group walks its own contiguous piece
            const gf_f32x4 *yr = reinterpret_cast<const gf_f32x4 *>(st + row * RS + seg * L);
            if constexpr (B == 32) {
                gf_f32x16 acc;
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[q] = 0.f;
#pragma unroll 4
                for (int j = 0; j < L / 4; ++j) {
                    const gf_f32x4 y = yr[j];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(y.x, y.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(y.y, y.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(y.z, y.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(y.w, y.w, acc, 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) Gs[((q & 3) + 8 * (q >> 2) + 4 * seg) * B + row] = acc[q];      // C/D map of the 32x32 MFMA
            } else {
                gf_f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};     // two accumulators: the 16x16x4 form issues faster than it completes
#pragma unroll 4
                for (int j = 0; j < L / 4; ++j) {
                    const gf_f32x4 y = yr[j];
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y.x, y.x, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y.y, y.y, acc1, 0, 0, 0);
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(y.z, y.z, acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(y.w, y.w, acc1, 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) Gs[(4 * seg + q) * B + row] = __fadd_rn(acc0[q], acc1[q]);       // C/D map of the 16x16 MFMA
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (lane == 0) gf_flag_st(&ready[sb], t + 1);
        }
    }
}

template <int VEC, int NV>
void launch_hub_block(const gemhip_gf_plan *p, int64_t row0, int64_t nhub, const float *Xold, float *Xnew, float eta, float regu, const GfHubDecay &dec,
                      hipStream_t s)
{
    // wavefronts per hub row: launch_hub's switch (8 or 4 with the chain's), read per launch here (tests change it in one process); the result does
    // not depend on it
    const char *env = getenv("GEMHIP_GF_HUB_PRODUCERS");
    const int np = env ? atoi(env) : 7;
    if (np >= 7)
        hipLaunchKernelGGL((gf_hub_block_kernel<VEC, NV, 7>), dim3((unsigned)nhub), dim3(512), 0, s, p->d_rows, p->d_ptr, p->d_col, p->d_w, Xold, Xnew,
                           row0, (int)p->d, eta, regu, dec);
    else
        hipLaunchKernelGGL((gf_hub_block_kernel<VEC, NV, 3>), dim3((unsigned)nhub), dim3(256), 0, s, p->d_rows, p->d_ptr, p->d_col, p->d_w, Xold, Xnew,
                           row0, (int)p->d, eta, regu, dec);
}

// ---- unit schedule (any edge order; gemhip_gf_plan_create_any_order).  A UNIT is a run of one row's edges that one wavefront applies in file order:
// it loads the row once -- from X_new when the row was already written in this sweep (bit 31 of its entry), else from X_old --, gathers every
// neighbour from the table bit 31 of d_col names, and stores the row to X_new.  Units of one level touch no common row that one of them writes.
// Same gf_apply_edge / gf_chunk as the row kernels: per edge the arithmetic is theirs bit for bit.  A unit of any length runs here (no hub path).
template <int VEC, int NV>
__device__ __forceinline__ void gf_unit_body(const uint32_t *__restrict__ units, const int64_t *__restrict__ ptr, const uint32_t *__restrict__ col,
                                             const float *__restrict__ w, const float *Xold, float *Xnew, int64_t u, int d, int lane, float eta,
                                             float regu)
{
    const uint32_t ru = units[u];
    const int64_t i = (int64_t)(ru & 0x7fffffffu);
    const int64_t e0 = ptr[u], e1 = ptr[u + 1];
    float xi[NV][VEC];
    const float *pi = ((ru >> 31) ? Xnew : Xold) + i * d;
#pragma unroll
    for (int c = 0; c < NV; ++c) load_row<VEC>(pi, d, lane, c, xi[c]);
    gf_row_edges<VEC, NV>(xi, e0, e1, col, w, Xold, Xnew, d, lane, eta, regu, 0);
    store_row<VEC, NV>(Xnew + i * d, d, lane, xi, 0);
}

// The units [unit0, unit0 + nunits) of ONE level, one wavefront each.
template <int VEC, int NV>
__global__ __launch_bounds__(GF_BLOCK) void gf_sweep_units_kernel(const uint32_t *__restrict__ units, const int64_t *__restrict__ ptr,
                                                                  const uint32_t *__restrict__ col, const float *__restrict__ w,
                                                                  const float *Xold, float *Xnew, int64_t unit0, int64_t nunits, int d,
                                                                  float eta, float regu)
{
    const int64_t slot = xcd_contiguous_block(blockIdx.x, gridDim.x) * GF_WAVES + (threadIdx.x >> 6);
    if (slot >= nunits) return;
    gf_unit_body<VEC, NV>(units, ptr, col, w, Xold, Xnew, unit0 + slot, d, lane_id(), eta, regu);
}

// The consecutive levels [l0, l1), each of at most GF_FUSED_WAVES units, in ONE launch of ONE workgroup: wavefront k runs unit k of the level, a
// workgroup barrier stands where the level loop has a kernel boundary.  The workgroup's wavefronts share one CU and its vector L1, so the barrier (with
// the workgroup-scope release / acquire __syncthreads carries: every store has left the wavefront before anyone passes) is all the ordering the rows
// handed from level to level need.  Every wavefront executes every barrier: l0, l1 are kernel arguments, and the test `k < units of the level`
// guards the unit body only.  Interleaving that comes from appended or concatenated files gives dozens of such levels in a row.
constexpr int GF_FUSED_WAVES = 16;
template <int VEC, int NV>
__global__ __launch_bounds__(GF_FUSED_WAVES * WAVE) void gf_units_fused_kernel(const uint32_t *__restrict__ units, const int64_t *__restrict__ ptr,
                                                                               const uint32_t *__restrict__ col, const float *__restrict__ w,
                                                                               const int64_t *__restrict__ level_off, const float *Xold, float *Xnew,
                                                                               int l0, int l1, int d, float eta, float regu)
{
    const int lane = lane_id();
    const int wave = threadIdx.x >> 6;
    for (int l = l0; l < l1; ++l) {
        const int64_t u0 = level_off[l], nu = level_off[l + 1] - u0;
        if (wave < nu) gf_unit_body<VEC, NV>(units, ptr, col, w, Xold, Xnew, u0 + wave, d, lane, eta, regu);
        __syncthreads();
    }
}

template <int VEC, int NV>
void launch_units(const gemhip_gf_plan *p, int64_t unit0, int64_t nunits, const float *Xold, float *Xnew, float eta, float regu, hipStream_t s)
{
    const int32_t *units = p->d_rows;
    hipLaunchKernelGGL((gf_sweep_units_kernel<VEC, NV>), gf_grid(nunits), dim3(GF_BLOCK), 0, s, (const uint32_t *)units, p->d_ptr, p->d_col,
                       p->d_w, Xold, Xnew, unit0, nunits, (int)p->d, eta, regu);
}
template <int VEC, int NV>
void launch_units_fused(const gemhip_gf_plan *p, int l0, int l1, const float *Xold, float *Xnew, float eta, float regu, hipStream_t s)
{
    const int32_t *units = p->d_rows;
    hipLaunchKernelGGL((gf_units_fused_kernel<VEC, NV>), dim3(1), dim3(GF_FUSED_WAVES * WAVE), 0, s, (const uint32_t *)units, p->d_ptr, p->d_col,
                       p->d_w, p->d_level_off, Xold, Xnew, l0, l1, (int)p->d, eta, regu);
}

// ---- one dispatch: the launchers of the (VEC, NV) instantiation a width d runs on.  A lane holds VEC floats of each of NV 64-lane chunks of a row:
// even d -> float2 per lane and ceil(d / 128) chunks, odd d -> one float and ceil(d / 64) chunks, the chunk count rounded up to 1, 2, 4 or 8.
struct gf_launchers {
    void (*sweep)(const gemhip_gf_plan *, int, int64_t, int64_t, const float *, float *, float, float, hipStream_t);
    void (*hub)(const gemhip_gf_plan *, int64_t, int64_t, const float *, float *, float, float, hipStream_t);
    void (*hub_block)(const gemhip_gf_plan *, int64_t, int64_t, const float *, float *, float, float, const GfHubDecay &, hipStream_t);
    int hub_block_edges;      // B of gf_hub_block_kernel at this width
    int (*coop)(const gemhip_gf_plan *, float *, float *, float, float, int, hipStream_t);
    void (*units)(const gemhip_gf_plan *, int64_t, int64_t, const float *, float *, float, float, hipStream_t);
    void (*units_fused)(const gemhip_gf_plan *, int, int, const float *, float *, float, float, hipStream_t);
};
template <int VEC, int NV> const gf_launchers *gf_launchers_of()
{
    static const gf_launchers L = {launch_sweep<VEC, NV>, launch_hub<VEC, NV>, launch_hub_block<VEC, NV>, gf_hub_block_cfg<VEC, NV, 7>::B,
                                   launch_coop<VEC, NV>, launch_units<VEC, NV>, launch_units_fused<VEC, NV>};
    return &L;
}
template <int VEC> const gf_launchers *gf_launchers_of_chunks(int nv)
{
    return nv <= 1 ? gf_launchers_of<VEC, 1>() : nv <= 2 ? gf_launchers_of<VEC, 2>() : nv <= 4 ? gf_launchers_of<VEC, 4>() : nv <= 8 ? gf_launchers_of<VEC, 8>() : nullptr;
}
// nullptr: d unsupported (supported: even d <= 1024, odd d <= 512)
const gf_launchers *gf_launchers_for(int d)
{
    if (d < 1) return nullptr;
    return d % 2 == 0 ? gf_launchers_of_chunks<2>((d + 127) / 128) : gf_launchers_of_chunks<1>((d + 63) / 64);
}

// 0.01*N(0,1)-style init: thread t fills elements 4t..4t+3 from one Philox block.
__global__ void gf_init_kernel(float *X, int64_t total, uint64_t seed, float scale)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t base = t * 4;
    if (base >= total) return;
    const u32x4 r = philox4x32_10(seed, (uint32_t)t, (uint32_t)(t >> 32), 0x6766u /* 'gf' */, 0u);
    const float u1 = 1.0f - u01(r.x), u2 = u01(r.y), u3 = 1.0f - u01(r.z), u4 = u01(r.w);   // (0,1]
    const float ra = sqrtf(-2.0f * logf(u1)), rb = sqrtf(-2.0f * logf(u3));
    float s0, c0, s1, c1;
    sincosf(6.28318530717958647692f * u2, &s0, &c0);
    sincosf(6.28318530717958647692f * u4, &s1, &c1);
    const float z[4] = {ra * c0, ra * s0, rb * c1, rb * s1};
    for (int k = 0; k < 4; ++k)
        if (base + k < total) X[base + k] = scale * z[k];
}

// gf.cpp:94-113 -- f1 = sum_e (w - X_i.X_j)^2 over ALL edges, f2 = ||X||_F^2.  One wave per edge.
__global__ __launch_bounds__(256) void gf_objective_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ dst,
                                                           const float *__restrict__ w, const float *__restrict__ X, int64_t m,
                                                           int64_t n, int d, double *out)
{
    const int lane = lane_id();
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    double f1 = 0.0, f2 = 0.0;
    for (int64_t e = wave0; e < m; e += nwaves) {
        const float *xi = X + (int64_t)src[e] * d, *xj = X + (int64_t)dst[e] * d;
        float part = 0.f;
        for (int k = lane; k < d; k += WAVE) part += xi[k] * xj[k];
        const float r = (w ? w[e] : 1.0f) - wave_sum(part);
        f1 += (double)r * (double)r;
    }
    for (int64_t v = wave0; v < n; v += nwaves) {
        const float *x = X + v * d;
        float part = 0.f;
        for (int k = lane; k < d; k += WAVE) part += x[k] * x[k];
        f2 += (double)wave_sum(part);
    }
    if (lane == 0) {
        atomicAdd(out, f1);
        atomicAdd(out + 1, f2);
    }
}

}  // namespace

// ------------------------------------------------------------------- host API
constexpr int GF_FUSED_LEVELS_DEFAULT = 16;

// what both creators check before they plan
static int gf_validate(const char *who, int64_t n, int64_t m, const int32_t *src, const int32_t *dst, gemhip_gf_plan_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "%s: out is NULL", who);
    *out = nullptr;
    GEMHIP_REQUIRE(n > 0 && n < (int64_t)0x7fffffff, "%s: n=%lld out of range", who, (long long)n);
    GEMHIP_REQUIRE(m >= 0 && (m == 0 || (src && dst)), "%s: bad edge arrays", who);
    return GEMHIP_OK;
}

// a planner's refusal in words
static int gf_plan_refused(const char *who, const GfPlanError &err, int64_t n, const int32_t *src, const int32_t *dst)
{
    const long long e = (long long)err.edge;
    switch (err.kind) {
    case GfPlanError::EDGE_OUT_OF_RANGE:
        return fail(GEMHIP_E_INVALID, "%s: edge %lld = (%d,%d) outside [0,%lld)", who, e, src[err.edge], dst[err.edge], (long long)n);
    case GfPlanError::PARTLY_UPDATED:
        return fail(GEMHIP_E_INVALID, "%s: edge %lld = (%d,%d) reads row %d while that row is only partly updated in file order "
                    "(its firing edges span positions %lld..%lld); the sequential semantics of gf.cpp need the edges of a source "
                    "to be contiguous (graph.edges() order) -- group the list by source first if the reordering is acceptable",
                    who, e, src[err.edge], dst[err.edge], dst[err.edge], (long long)err.first, (long long)err.last);
    case GfPlanError::TOO_MANY_UNITS: return fail(GEMHIP_E_INVALID, "%s: more than 2^31 - 1 units", who);
    default: return GEMHIP_OK;
    }
}

// the host plan H (planned since t_host0) becomes a device plan: H's small vectors move into it, its arrays are uploaded
static int gf_plan_upload(const char *who, int64_t n, int32_t d, GfHostPlan &H, double t_host0, gemhip_gf_plan_t *out)
{
    auto *p = new gemhip_gf_plan();
    p->n = n; p->d = d; p->fn = gf_launchers_for(d);
    p->nrows = H.nrows; p->nupd = H.nupd; p->units = H.units;
    p->level_off.swap(H.level_off); p->level_hubs.swap(H.level_hubs); p->level_maxlen.swap(H.level_maxlen); p->segs.swap(H.segs);
    if (hipGetDevice(&p->device) != hipSuccess) { delete p; return fail(GEMHIP_E_HIP, "%s: no HIP device", who); }
    phase_acc()[PH_HOST] += phase_now() - t_host0;
    PhaseScope ph_up(PH_H2D);
    hipError_t e = p->d_rows.upload(H.rows.data(), H.nrows);
    if (e == hipSuccess) e = p->d_ptr.upload(H.ptr.data(), H.nrows + 1);
    if (e == hipSuccess) e = p->d_col.upload(H.col.data(), H.nupd);
    if (e == hipSuccess) e = p->d_w.upload(H.w.data(), H.nupd);
    if (e == hipSuccess && H.units) e = p->d_level_off.upload(p->level_off.data(), p->level_off.size());
    if (e != hipSuccess) {
        gemhip_gf_plan_destroy(p);
        return fail(GEMHIP_E_HIP, "%s: device upload failed: %s", who, hipGetErrorString(e));
    }
    *out = p;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_create(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d,
                                     int64_t row_begin, int64_t row_end, gemhip_gf_plan_t *out)
{
    const char *who = "gf_plan_create";
    if (int rc = gf_validate(who, n, m, src, dst, out)) return rc;
    GEMHIP_REQUIRE(d >= 1, "gf_plan_create: d=%d", d);
    GEMHIP_REQUIRE(gf_launchers_for(d) != nullptr, "gf_plan_create: d=%d unsupported (even d <= 1024, odd d <= 512)", d);
    GEMHIP_REQUIRE(0 <= row_begin && row_begin <= row_end && row_end <= n, "gf_plan_create: bad row range");
    const double t_host0 = phase_now();
    // rows with at least this many firing edges get a workgroup (gf_hub_kernel); 0: none do.  Read per call (tests lower it)
    const int64_t hub_edges = getenv("GEMHIP_GF_NO_HUB_KERNEL") ? 0 : getenv("GEMHIP_GF_HUB_EDGES") ? std::max(1, atoi(getenv("GEMHIP_GF_HUB_EDGES"))) : GF_HUB_EDGES;
    GfHostPlan H;
    // a list that needs an intermediate version of a row is rejected instead of silently reordered
    if (const GfPlanError err = gf_plan_rows(n, m, src, dst, w, row_begin, row_end, hub_edges, H)) return gf_plan_refused(who, err, n, src, dst);
    return gf_plan_upload(who, n, d, H, t_host0, out);
}

extern "C" int gemhip_gf_any_order_schedule(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, int32_t *unit_out, int32_t *level_out,
                                            int32_t *flags_out, int64_t *counts)
{
    GEMHIP_REQUIRE(n > 0 && n < (int64_t)0x7fffffff, "gf_any_order_schedule: n=%lld out of range", (long long)n);
    GEMHIP_REQUIRE(m >= 0 && (m == 0 || (src && dst)), "gf_any_order_schedule: bad edge arrays");
    GfUnitSchedule S;
    if (const GfPlanError err = gf_schedule_units(n, m, src, dst, S)) return gf_plan_refused("gf_any_order_schedule", err, n, src, dst);
    for (int64_t e = 0; e < m; ++e) {
        const int32_t u = S.unit_of[e];
        if (unit_out) unit_out[e] = u;
        if (level_out) level_out[e] = u < 0 ? -1 : S.level[u];
        if (flags_out) flags_out[e] = u < 0 ? -1 : (int32_t)S.nb_new[e] | ((int32_t)S.own_new[u] << 1);
    }
    if (counts) { counts[0] = (int64_t)S.row.size(); counts[1] = S.nlevels; }
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_create_any_order(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d,
                                               int32_t flags, gemhip_gf_plan_t *out)
{
    const char *who = "gf_plan_create_any_order";
    if (int rc = gf_validate(who, n, m, src, dst, out)) return rc;
    GEMHIP_REQUIRE(gf_launchers_for(d) != nullptr, "gf_plan_create_any_order: d=%d unsupported (even d <= 1024, odd d <= 512)", d);
    GEMHIP_REQUIRE((flags & ~1) == 0, "gf_plan_create_any_order: flags=%d (bit 0 = force the unit schedule)", flags);
    // a list the row schedule represents gets exactly that plan: same levels, same kernels, same speed (and one with an endpoint out of range
    // goes there too: that call reports it)
    if (!(flags & 1) && gf_check_row_order(n, m, src, dst).kind != GfPlanError::PARTLY_UPDATED) return gemhip_gf_plan_create(n, m, src, dst, w, d, 0, n, out);
    const double t_host0 = phase_now();
    GfHostPlan H;
    if (const GfPlanError err = gf_plan_units(n, m, src, dst, w, GF_FUSED_LEVELS_DEFAULT, H)) return gf_plan_refused(who, err, n, src, dst);
    return gf_plan_upload(who, n, d, H, t_host0, out);
}

extern "C" int gemhip_gf_plan_set_fused_levels(gemhip_gf_plan_t p, int32_t max_units)
{
    GEMHIP_REQUIRE(p && max_units >= 0 && max_units <= GF_FUSED_WAVES, "gf_plan_set_fused_levels: 0 (off) .. %d units", GF_FUSED_WAVES);
    if (p->units) p->segs = gf_units_segments(p->level_off, max_units);
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_destroy(gemhip_gf_plan_t p)
{
    if (!p) return GEMHIP_OK;
    if (p->hub_stream) { hipStreamSynchronize(p->hub_stream); hipStreamDestroy(p->hub_stream); hipEventDestroy(p->hub_fork); hipEventDestroy(p->hub_join); }
    delete p;
    return GEMHIP_OK;
}

static int ensure_tables(gemhip_gf_plan_t p)
{
    if (p->X[0]) return GEMHIP_OK;
    for (int k = 0; k < 2; ++k) GEMHIP_CHECK(p->X_own[k].reserve((size_t)p->n * p->d));
    p->X[0] = p->X_own[0]; p->X[1] = p->X_own[1]; p->cur = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_bind(gemhip_gf_plan_t p, void *dXa, void *dXb)
{
    GEMHIP_REQUIRE(p && dXa && dXb && dXa != dXb, "gf_plan_bind: need two distinct device buffers");
    p->X_own[0].reset(); p->X_own[1].reset();
    p->X[0] = (float *)dXa; p->X[1] = (float *)dXb; p->cur = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_set_embedding(gemhip_gf_plan_t p, const float *X_host)
{
    GEMHIP_REQUIRE(p && X_host, "gf_plan_set_embedding: NULL argument");
    if (int rc = ensure_tables(p)) return rc;
    const size_t bytes = (size_t)p->n * p->d * sizeof(float);
    PhaseScope ph(PH_H2D);
    GEMHIP_CHECK(hipMemcpy(p->X[0], X_host, bytes, hipMemcpyHostToDevice));
    GEMHIP_CHECK(hipMemcpy(p->X[1], p->X[0], bytes, hipMemcpyDeviceToDevice));
    p->cur = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_init_embedding(gemhip_gf_plan_t p, uint64_t seed, float scale)
{
    GEMHIP_REQUIRE(p, "gf_plan_init_embedding: NULL plan");
    if (int rc = ensure_tables(p)) return rc;
    const int64_t total = p->n * p->d;
    const int64_t threads = (total + 3) / 4;
    hipLaunchKernelGGL(gf_init_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, p->X[0], total, seed, scale);
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipMemcpy(p->X[1], p->X[0], (size_t)total * sizeof(float), hipMemcpyDeviceToDevice));
    p->cur = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_sweeps(gemhip_gf_plan_t p, int32_t nsweeps, float eta, float regu, void *stream)
{
    GEMHIP_REQUIRE(p && nsweeps >= 0, "gf_plan_sweeps: bad arguments");
    GEMHIP_REQUIRE(p->X[0] && p->X[1], "gf_plan_sweeps: no embedding table (call set/init/bind first)");
    if (p->nrows == 0) return GEMHIP_OK;
    hipStream_t s = (hipStream_t)stream;
    if (p->units) {                                    // unit schedule: the launches of gf_units_segments, in stream order
        for (int it = 0; it < nsweeps; ++it) {
            const float *Xold = p->X[p->cur];
            float *Xnew = p->X[p->cur ^ 1];
            for (const auto &g : p->segs) {
                if (g.fused) p->fn->units_fused(p, g.l0, g.l1, Xold, Xnew, eta, regu, s);
                else p->fn->units(p, p->level_off[g.l0], p->level_off[g.l1] - p->level_off[g.l0], Xold, Xnew, eta, regu, s);
            }
            p->cur ^= 1;
        }
        GEMHIP_CHECK(hipGetLastError());
        return GEMHIP_OK;
    }
    const int nlevels = (int)p->level_off.size() - 1;
    GfHubDecay decay;                                  // the powers of 1 - eta * regu the blocked hub kernel scales with: eta and regu arrive here
    if (p->hub_block) {
        GEMHIP_REQUIRE(p->fn->hub_block_edges == gf_hub_block((int)p->d), "gf_plan_sweeps: block size of d=%lld", (long long)p->d);
        gf_hub_decay(eta, regu, p->fn->hub_block_edges, decay.hi, decay.lo);
    }
    int it0 = 0;
    if (p->fused_sweeps > 1 && nlevels == 1 && (p->level_hubs.empty() || p->level_hubs[0] == 0)) {
        // up to fused_sweeps sweeps per cooperative launch; the table of sweep k is X[cur ^ (k & 1)]
        while (nsweeps - it0 >= 2) {
            const int k = std::min(nsweeps - it0, p->fused_sweeps);
            if (int rc = p->fn->coop(p, p->X[p->cur], p->X[p->cur ^ 1], eta, regu, k, s)) return rc;
            if (k & 1) p->cur ^= 1;
            it0 += k;
        }
    }
    for (int it = it0; it < nsweeps; ++it) {
        const float *Xold = p->X[p->cur];
        float *Xnew = p->X[p->cur ^ 1];
        for (int l = 0; l < nlevels; ++l) {
            const int64_t r0 = p->level_off[l], nr = p->level_off[l + 1] - r0;
            const int64_t nh = l < (int)p->level_hubs.size() ? p->level_hubs[l] : 0;
            if (nh > 0) {                              // hub rows of this level on a side stream, next to the wave-per-row kernel
                if (!p->hub_stream) {
                    GEMHIP_CHECK(hipStreamCreateWithFlags(&p->hub_stream, hipStreamNonBlocking));
                    GEMHIP_CHECK(hipEventCreateWithFlags(&p->hub_fork, hipEventDisableTiming));
                    GEMHIP_CHECK(hipEventCreateWithFlags(&p->hub_join, hipEventDisableTiming));
                }
                GEMHIP_CHECK(hipEventRecord(p->hub_fork, s));
                GEMHIP_CHECK(hipStreamWaitEvent(p->hub_stream, p->hub_fork, 0));
                if (p->hub_block) p->fn->hub_block(p, r0, nh, Xold, Xnew, eta, regu, decay, p->hub_stream);
                else p->fn->hub(p, r0, nh, Xold, Xnew, eta, regu, p->hub_stream);
                GEMHIP_CHECK(hipEventRecord(p->hub_join, p->hub_stream));
            }
            if (nr - nh > 0) p->fn->sweep(p, l, r0 + nh, nr - nh, Xold, Xnew, eta, regu, s);
            if (nh > 0) GEMHIP_CHECK(hipStreamWaitEvent(s, p->hub_join, 0));
        }
        p->cur ^= 1;
    }
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_set_rows_per_wave(gemhip_gf_plan_t p, int32_t rows_per_wave)
{
    GEMHIP_REQUIRE(p && rows_per_wave >= 0 && rows_per_wave <= 64, "gf_plan_set_rows_per_wave: 0 (auto) .. 64");
    p->rows_per_wave = rows_per_wave;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_set_fused_sweeps(gemhip_gf_plan_t p, int32_t sweeps_per_launch, int32_t max_grid)
{
    GEMHIP_REQUIRE(p && sweeps_per_launch >= 0 && sweeps_per_launch <= 65536 && max_grid >= 0, "gf_plan_set_fused_sweeps: bad arguments");
    p->fused_sweeps = sweeps_per_launch; p->fused_grid = max_grid;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_set_hub_block(gemhip_gf_plan_t p, int32_t on)
{
    GEMHIP_REQUIRE(p && (on == 0 || on == 1), "gf_plan_set_hub_block: 0 (off) or 1 (on)");
    if (!p->units) p->hub_block = on;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_hub_block(gemhip_gf_plan_t p, int32_t *block, int64_t *hub_rows)
{
    GEMHIP_REQUIRE(p && block && hub_rows, "gf_plan_hub_block: NULL argument");
    *block = (p->units || !p->hub_block) ? 0 : p->fn->hub_block_edges;
    *hub_rows = 0;
    for (int64_t h : p->level_hubs) *hub_rows += h;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_get_embedding(gemhip_gf_plan_t p, float *X_host)
{
    GEMHIP_REQUIRE(p && X_host && p->X[0], "gf_plan_get_embedding: bad arguments");
    GEMHIP_CHECK(hipDeviceSynchronize());
    PhaseScope ph(PH_D2H);
    GEMHIP_CHECK(hipMemcpy(X_host, p->X[p->cur], (size_t)p->n * p->d * sizeof(float), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_current(gemhip_gf_plan_t p, void **dX)
{
    GEMHIP_REQUIRE(p && dX, "gf_plan_current: NULL argument");
    *dX = p->X[p->cur];
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_plan_info(gemhip_gf_plan_t p, int64_t *info)
{
    GEMHIP_REQUIRE(p && info, "gf_plan_info: NULL argument");
    info[0] = p->nupd; info[1] = p->nrows; info[2] = (int64_t)p->level_off.size() - 1; info[3] = p->n; info[4] = p->d;
    // 3*4d + 12 bytes per update (read X_i, read X_j, write X_i, (i,j,w))
    info[5] = p->nupd * (3 * 4 * p->d + 12);
    {   // rows per wavefront the largest level's sweep launch will use (1: gf_sweep_kernel, > 1: gf_sweep_rows_kernel); of equally large levels: the last
        int64_t big = 0;
        size_t lbig = p->level_off.size();                       // (no level: the rule on an empty one)
        for (size_t l = 0; l + 1 < p->level_off.size(); ++l)
            if (p->level_off[l + 1] - p->level_off[l] >= big) { big = p->level_off[l + 1] - p->level_off[l]; lbig = l; }
        info[6] = p->units ? 1 : gf_rows_per_wave(p, lbig, big);
    }
    info[7] = p->units ? 1 : 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_gf_train(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d, float eta,
                               float regu, int32_t max_iter, float *X_inout, double *stats)
{
    GEMHIP_REQUIRE(X_inout != nullptr, "gf_train: X_inout is NULL");
    GEMHIP_REQUIRE(max_iter >= 0, "gf_train: max_iter=%d", max_iter);
    for (int k = 0; k < PH_COUNT; ++k) phase_acc()[k] = 0.0;
    const double t_call = phase_now();
    gemhip_gf_plan_t p = nullptr;
    int rc = gemhip_gf_plan_create(n, m, src, dst, w, d, 0, n, &p);
    if (rc) return rc;
    rc = gemhip_gf_plan_set_embedding(p, X_inout);
    EventMarks<2> t;
    double ms = 0.0;
    if (!rc && t.create() != hipSuccess) rc = fail(GEMHIP_E_HIP, "gf_train: hipEventCreate");
    if (!rc) {
        (void)t.mark(0);
        rc = gemhip_gf_plan_sweeps(p, max_iter, eta, regu, nullptr);
        (void)t.mark(1);
    }
    if (!rc) rc = gemhip_gf_plan_get_embedding(p, X_inout);
    if (!rc) (void)t.ms(0, 1, &ms);
    phase_acc()[PH_KERNELS] = ms * 1e-3;
    if (stats && !rc) {
        stats[0] = ms * 1e-3; stats[1] = (double)p->nupd; stats[2] = (double)p->nrows;
        stats[3] = (double)(p->level_off.size() - 1);
    }
    gemhip_gf_plan_destroy(p);
    phase_acc()[PH_TOTAL] = phase_now() - t_call;
    return rc;
}

extern "C" int gemhip_gf_objective(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d,
                                   const float *X_host, double *out)
{
    GEMHIP_REQUIRE(n > 0 && m >= 0 && d >= 1 && X_host && out, "gf_objective: bad arguments");
    GEMHIP_REQUIRE(m == 0 || (src && dst), "gf_objective: bad edge arrays");
    for (int64_t e = 0; e < m; ++e)                          // the kernel reads rows src[e], dst[e] of X unchecked
        GEMHIP_REQUIRE(src[e] >= 0 && src[e] < n && dst[e] >= 0 && dst[e] < n, "gf_objective: edge %lld = (%d,%d) outside [0,%lld)", (long long)e, src[e],
                       dst[e], (long long)n);
    DevBuf<int32_t> ds, dd; DevBuf<float> dw, dX; DevBuf<double> dout;
    GEMHIP_CHECK(ds.upload(src, m));
    GEMHIP_CHECK(dd.upload(dst, m));
    if (w) GEMHIP_CHECK(dw.upload(w, m));
    GEMHIP_CHECK(dX.upload(X_host, (size_t)n * d));
    GEMHIP_CHECK(dout.reserve(2));
    GEMHIP_CHECK(hipMemset(dout, 0, 16));
    hipLaunchKernelGGL(gf_objective_kernel, dim3(2048), dim3(256), 0, 0, ds, dd, dw, dX, m, n, (int)d, dout);
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipMemcpy(out, dout, 16, hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}
