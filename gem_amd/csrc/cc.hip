// cc.hip -- weakly connected components of an arc list and its largest component, relabelled (gemhip_cc_labels, gemhip_lcc).
// Replaces gem/utils/graph_util.py:29-34 (get_lcc: largest weakly connected component, nodes renumbered 0..k-1), which upstream GEM's
// link-prediction driver applies to the train half of every split.
//
// Pipeline (every phase is its own kernel launch on the null stream; the kernel boundary is the only synchronisation there is):
//   cc_init_kernel      parent[v] = v
//   cc_union_kernel     one thread per arc: lock-free union-find, larger root hooked under the smaller by atomicCAS
//   cc_flatten_kernel   label[v] = root(v)                                   -> the component's smallest node id
//   cc_sizes_kernel     size[label[v]] += 1, aggregated inside a wavefront   -> one atomic per distinct label per wavefront
//   cc_winner_kernel    arg-max of (size, then smallest label) over the roots, and the number of roots
//   cc_count / cc_scan_sums / cc_scatter_*   stable compaction of the kept nodes, then of the kept arcs (three-kernel exclusive scans)
//
// Why the union is correct although it reads parent[] without a lock and possibly stale
// -----------------------------------------------------------------------------------
// (I)   Every value ever stored in parent[v] is <= v.  cc_init stores v; the only other store is a successful
//       atomicCAS(&parent[hi], hi, lo) with lo < hi.  Hence parent pointers strictly decrease along a path until a root (parent[r] == r):
//       the pointers never form a cycle, and the root of a tree is the smallest id in it.
// (II)  parent[v] changes at most once: from v (root) to some lo < v, by the one CAS that finds it equal to v.  A node that stopped being a
//       root never becomes one again and its pointer is final.  So the only two values a load of parent[v] can ever return are v and that
//       final lo -- "an older value" means v itself.
// (III) gfx950's per-CU L1 is not coherent with other CUs: a load may return the older value v after another CU has hooked v.  (The find
//       loop uses relaxed agent-scope loads, which are served by L2 and are fresher, but nothing below needs that.)  By (II) the reader
//       then takes v for a root.  v is still a node of the same tree as the arc's end it started from (edges are never removed), and
//       v <= the node it came from: the two facts the algorithm uses.  It is a legitimate, if not final, representative.
// (IV)  The CAS executes at the memory side (L2 / fabric atomics), on the one true copy of parent[hi].  It succeeds only if hi is a root
//       at that instant; a thread that took a hooked node for a root fails here, receives the true parent (< hi) and continues from it.
//       A successful CAS hooks a true root hi under lo, a node of the OTHER end's tree with lo < hi: the two trees become one and (I) holds.
// (V)   Termination, per thread and with no thread waiting for any other: the find loop moves to a strictly smaller id at every step
//       (I); the link loop either succeeds in its CAS (done), or finds both ends at one node (done: same tree), or replaces hi by a
//       strictly smaller id.  Ids are bounded below by 0.  There is no spin on a flag, no look-back, no grid barrier, no cooperative
//       launch: a thread whose CAS failed does new work with the value it got back, it never re-reads a location until it changes.
// (VI)  When a thread ends, both ends of its arc are in one tree (it saw a common node, or its CAS merged the trees), and trees are never
//       split.  After the kernel every arc joins one tree, so trees == weak components; cc_flatten runs behind the kernel boundary (all
//       stores visible, parent[] read-only) and writes the root = the component's smallest id.  Labels therefore do not depend on the order
//       in which threads ran: bit-identical from run to run, although the shape of the intermediate forest is not.
//
// Sizes, winner, compaction are integer counts and prefix sums: order-independent as well.
#include "common.hpp"
#include <climits>

using namespace gemhip;

namespace {

constexpr int CC_BLOCK = 256;                         // threads per workgroup of every kernel but cc_scan_sums_kernel
constexpr int CC_MAX_GRID = 1 << 16;                  // grid-stride kernels: workgroups at most
constexpr int SCAN_ITEMS = 4;                         // consecutive elements per thread in the count / scatter kernels
constexpr int SCAN_TILE = CC_BLOCK * SCAN_ITEMS;      // elements per workgroup: 1024
constexpr int SUMS_BLOCK = 1024;                      // cc_scan_sums_kernel: ONE workgroup, SUMS_BLOCK tile counts per pass

// What the kernels hand to each other and to the host: zeroed before the first launch.
struct CcScalars {
    unsigned long long best;       // max over roots of (size << 32) | (0xFFFFFFFF - label): the largest component, the smallest label on a tie
    int32_t n_components;
    int32_t n_kept, m_kept;        // totals of the two compactions
    int32_t pad;
};

__device__ __forceinline__ int32_t winner_of(const CcScalars *sc) { return (int32_t)(0xFFFFFFFFu - (uint32_t)(sc->best & 0xFFFFFFFFull)); }

__global__ __launch_bounds__(CC_BLOCK) void cc_init_kernel(int32_t *__restrict__ parent, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * CC_BLOCK;
    for (int64_t v = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x; v < n; v += stride) parent[v] = (int32_t)v;
}

// Follow parents from x to a node that reads as a root.  Every step goes to a strictly smaller id (header (I)), so it ends.
__device__ __forceinline__ int32_t cc_find(const int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

__global__ __launch_bounds__(CC_BLOCK) void cc_union_kernel(int32_t *parent, const int32_t *__restrict__ src, const int32_t *__restrict__ dst, int64_t m)
{
    const int64_t stride = (int64_t)gridDim.x * CC_BLOCK;
    for (int64_t e = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x; e < m; e += stride) {
        int32_t a = src[e], b = dst[e];
        if (a == b) continue;                                   // self-loop
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        while (a != b) {                                        // a == b: one tree already
            const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
            const int32_t seen = atomicCAS(parent + hi, hi, lo);
            if (seen == hi) break;                              // hi was a root and now hangs under lo
            a = cc_find(parent, seen);                          // hi had a parent already: seen < hi, go on from there
            b = lo;
        }
    }
}

__global__ __launch_bounds__(CC_BLOCK) void cc_flatten_kernel(const int32_t *__restrict__ parent, int32_t *__restrict__ label, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * CC_BLOCK;
    for (int64_t v = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x; v < n; v += stride) {
        int32_t x = (int32_t)v;
        for (int32_t p = parent[x]; p != x; p = parent[x]) x = p;
        label[v] = x;
    }
}

// size[label[v]] += 1.  The giant component would put nearly every add on one address, so a wavefront first groups its 64 labels: the first lane
// still to be counted names its label, the lanes holding the same label are found with one ballot and leave together, that first lane adds
// their number.  One atomic per distinct label per wavefront -- 1 in the giant component, up to 64 in debris (then 64 different addresses).
__global__ __launch_bounds__(CC_BLOCK) void cc_sizes_kernel(const int32_t *__restrict__ label, int32_t *size, int64_t n)
{
    const int lane = lane_id();
    const int64_t stride = (int64_t)gridDim.x * CC_BLOCK;
    for (int64_t base = (int64_t)blockIdx.x * CC_BLOCK + (threadIdx.x - lane); base < n; base += stride) {      // base: the same in all lanes of a wavefront
        const int64_t v = base + lane;
        const bool have = v < n;
        const int32_t mine = have ? label[v] : -1;
        unsigned long long todo = __ballot(have);
        while (todo) {                                                                                           // (the same in all lanes)
            const int first = __ffsll(todo) - 1;
            const int32_t named = __shfl(mine, first);
            const unsigned long long same = __ballot(have && mine == named);
            if (lane == first) atomicAdd(size + named, (int32_t)__popcll(same));
            todo &= ~same;
        }
    }
}

// Over the roots (size > 0 exactly at v == label of a component): the number of them, and the maximum of (size, then SMALLEST label).
__global__ __launch_bounds__(CC_BLOCK) void cc_winner_kernel(const int32_t *__restrict__ size, int64_t n, CcScalars *sc)
{
    unsigned long long key = 0;
    int32_t roots = 0;
    const int64_t stride = (int64_t)gridDim.x * CC_BLOCK;
    for (int64_t v = (int64_t)blockIdx.x * CC_BLOCK + threadIdx.x; v < n; v += stride) {
        const int32_t s = size[v];
        if (s > 0) {
            const unsigned long long k = ((unsigned long long)(uint32_t)s << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)v);
            key = k > key ? k : key;
            ++roots;
        }
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const unsigned long long k = __shfl_down(key, off);
        key = k > key ? k : key;
        roots += __shfl_down(roots, off);
    }
    if (lane_id() == 0 && roots > 0) {
        atomicMax(&sc->best, key);
        atomicAdd(&sc->n_components, roots);
    }
}

// Exclusive prefix of `c` over the threads of a workgroup of BLOCK threads, in thread order; *total = the workgroup's sum.  Every thread calls it.
template <int BLOCK>
__device__ __forceinline__ int32_t block_exclusive_scan(int32_t c, int32_t *total)
{
    __shared__ int32_t wave_sum_of[BLOCK / WAVE];
    const int lane = lane_id(), wave = threadIdx.x / WAVE;
    int32_t incl = c;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int32_t t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == WAVE - 1) wave_sum_of[wave] = incl;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < BLOCK / WAVE; ++k) {
        const int32_t s = wave_sum_of[k];
        before += k < wave ? s : 0;
        all += s;
    }
    __syncthreads();                                            // the next call writes wave_sum_of again
    *total = all;
    return before + incl - c;
}

// What is kept.  Nodes: those of the winning component.  Arcs: those whose source is kept (its target then is too: one weak component).
struct KeepNode {
    const int32_t *label;
    __device__ bool operator()(int64_t v, int32_t winner) const { return label[v] == winner; }
};
struct KeepArc {
    const int32_t *src; const int32_t *new_of_old;
    __device__ bool operator()(int64_t e, int32_t) const { return new_of_old[src[e]] >= 0; }
};

// Scan, kernel 1 of 3: tile_count[t] = kept elements among the SCAN_TILE elements of tile t.
template <typename Keep>
__global__ __launch_bounds__(CC_BLOCK) void cc_count_kernel(Keep keep, const CcScalars *sc, int64_t count, int32_t *__restrict__ tile_count)
{
    const int32_t winner = winner_of(sc);
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (base + k < count) c += keep(base + k, winner) ? 1 : 0;
    int32_t total;
    block_exclusive_scan<CC_BLOCK>(c, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// Scan, kernel 2 of 3: ONE workgroup turns the tile counts into exclusive offsets in place, SUMS_BLOCK at a time with a running carry, and
// leaves the grand total in *total_out.
__global__ __launch_bounds__(SUMS_BLOCK) void cc_scan_sums_kernel(int32_t *tile_count, int64_t ntiles, int32_t *total_out)
{
    int32_t carry = 0;
    for (int64_t base = 0; base < ntiles; base += SUMS_BLOCK) {
        const int64_t t = base + threadIdx.x;
        const int32_t c = t < ntiles ? tile_count[t] : 0;
        int32_t total;
        const int32_t excl = block_exclusive_scan<SUMS_BLOCK>(c, &total);
        if (t < ntiles) tile_count[t] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// Scan, kernel 3 of 3, nodes: new_of_old[v] = rank of v among the kept nodes (ascending with v) or -1, old_of_new = its inverse.
__global__ __launch_bounds__(CC_BLOCK) void cc_scatter_nodes_kernel(KeepNode keep, const CcScalars *sc, int64_t n, const int32_t *__restrict__ tile_offset,
                                                                    int32_t *__restrict__ new_of_old, int32_t *__restrict__ old_of_new)
{
    const int32_t winner = winner_of(sc);
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    bool f[SCAN_ITEMS];
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        f[k] = base + k < n && keep(base + k, winner);
        c += f[k] ? 1 : 0;
    }
    int32_t total;
    int32_t at = tile_offset[blockIdx.x] + block_exclusive_scan<CC_BLOCK>(c, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k >= n) break;
        if (f[k]) { new_of_old[base + k] = at; old_of_new[at] = (int32_t)(base + k); ++at; }
        else new_of_old[base + k] = -1;
    }
}

// ... arcs: the kept arcs in their original order, both ends renumbered, the weight's 32 bits copied as they are.
__global__ __launch_bounds__(CC_BLOCK) void cc_scatter_arcs_kernel(KeepArc keep, int64_t m, const int32_t *__restrict__ dst, const uint32_t *__restrict__ w,
                                                                   const int32_t *__restrict__ tile_offset, int32_t *__restrict__ src_out,
                                                                   int32_t *__restrict__ dst_out, uint32_t *__restrict__ w_out)
{
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + (int64_t)threadIdx.x * SCAN_ITEMS;
    int32_t s_new[SCAN_ITEMS];
    int32_t c = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        s_new[k] = base + k < m ? keep.new_of_old[keep.src[base + k]] : -1;
        c += s_new[k] >= 0 ? 1 : 0;
    }
    int32_t total;
    int32_t at = tile_offset[blockIdx.x] + block_exclusive_scan<CC_BLOCK>(c, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        if (s_new[k] < 0) continue;
        src_out[at] = s_new[k];
        dst_out[at] = keep.new_of_old[dst[base + k]];
        if (w) w_out[at] = w[base + k];
        ++at;
    }
}

// ---------------------------------------------------------------- host side
int grid_for(int64_t count)
{
    const int64_t g = (count + CC_BLOCK - 1) / CC_BLOCK;
    return (int)(g < 1 ? 1 : g > CC_MAX_GRID ? CC_MAX_GRID : g);
}

// Kernel times of the last call on this thread (gemhip_cc_last_kernel_ms): HIP events between the launches.
enum { K_INIT = 0, K_UNION, K_FLATTEN, K_SIZES, K_WINNER, K_NODES, K_ARCS, K_COUNT };
double *kernel_ms() { static thread_local double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0}; return ms; }

struct Events {                                         // K_COUNT + 1 marks on the null stream, taken in order
    EventMarks<K_COUNT + 1> ev;
    int marked = 0;
    hipError_t create() { return ev.create(); }
    hipError_t mark() { return ev.mark(marked++); }
    hipError_t collect()                                // ms between consecutive marks
    {
        for (int k = 0; k + 1 < marked; ++k) {
            double ms = 0.0;
            const hipError_t r = ev.ms(k, k + 1, &ms);
            if (r != hipSuccess) return r;
            kernel_ms()[k] = ms;
            phase_acc()[PH_KERNELS] += ms * 1e-3;
        }
        return hipSuccess;
    }
};

int validate(const char *who, int64_t n, int64_t m, const int32_t *src, const int32_t *dst)
{
    GEMHIP_REQUIRE(n >= 1 && m >= 0, "%s: n = %lld, m = %lld (need n >= 1, m >= 0)", who, (long long)n, (long long)m);
    if (n > INT32_MAX || m > INT32_MAX)
        return fail(GEMHIP_E_UNSUPPORTED, "%s: n = %lld, m = %lld: both must be below 2^31", who, (long long)n, (long long)m);
    GEMHIP_REQUIRE(m == 0 || (src && dst), "%s: bad edge arrays", who);
    for (int64_t e = 0; e < m; ++e)                           // the kernels index parent[] and new_of_old[] with src[e], dst[e] unchecked
        GEMHIP_REQUIRE(src[e] >= 0 && src[e] < n && dst[e] >= 0 && dst[e] < n, "%s: edge %lld = (%d,%d) outside [0,%lld)", who, (long long)e, src[e], dst[e],
                       (long long)n);
    return GEMHIP_OK;
}

struct Device {                                         // everything a call holds on the device
    DevBuf<int32_t> src, dst, parent, label, size;
    DevBuf<CcScalars> sc;
    Events ev;
};

// Upload the arcs and enqueue init .. winner.  Leaves label[], size[] and *sc (best, n_components) to the launches that follow on the stream.
int enqueue_labels(Device &D, int64_t n, int64_t m, const int32_t *src, const int32_t *dst)
{
    {
        PhaseScope ph(PH_H2D);
        GEMHIP_CHECK(D.src.upload(src, (size_t)m));
        GEMHIP_CHECK(D.dst.upload(dst, (size_t)m));
    }
    GEMHIP_CHECK(D.parent.reserve((size_t)n));
    GEMHIP_CHECK(D.label.reserve((size_t)n));
    GEMHIP_CHECK(D.size.reserve((size_t)n));
    GEMHIP_CHECK(D.sc.reserve(1));
    GEMHIP_CHECK(D.ev.create());
    GEMHIP_CHECK(hipMemsetAsync(D.size, 0, (size_t)n * sizeof(int32_t), 0));
    GEMHIP_CHECK(hipMemsetAsync(D.sc, 0, sizeof(CcScalars), 0));
    GEMHIP_CHECK(D.ev.mark());
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid_for(n)), dim3(CC_BLOCK), 0, 0, D.parent.get(), n);
    GEMHIP_CHECK(D.ev.mark());
    if (m > 0) hipLaunchKernelGGL(cc_union_kernel, dim3(grid_for(m)), dim3(CC_BLOCK), 0, 0, D.parent.get(), D.src.get(), D.dst.get(), m);
    GEMHIP_CHECK(D.ev.mark());
    hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_for(n)), dim3(CC_BLOCK), 0, 0, D.parent.get(), D.label.get(), n);
    GEMHIP_CHECK(D.ev.mark());
    hipLaunchKernelGGL(cc_sizes_kernel, dim3(grid_for(n)), dim3(CC_BLOCK), 0, 0, D.label.get(), D.size.get(), n);
    GEMHIP_CHECK(D.ev.mark());
    const int winner_grid = grid_for(n) < 256 ? grid_for(n) : 256;          // one pair of atomics per wavefront: keep them few
    hipLaunchKernelGGL(cc_winner_kernel, dim3(winner_grid), dim3(CC_BLOCK), 0, 0, D.size.get(), n, D.sc.get());
    GEMHIP_CHECK(D.ev.mark());
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

// The three kernels of one compaction; `scatter` launches the third.
template <typename Keep, typename Scatter>
int enqueue_compaction(Keep keep, const CcScalars *sc, int64_t count, DevBuf<int32_t> &tiles, int32_t *total_out, Scatter scatter)
{
    const int64_t ntiles = (count + SCAN_TILE - 1) / SCAN_TILE;
    GEMHIP_CHECK(tiles.reserve((size_t)ntiles));
    hipLaunchKernelGGL(cc_count_kernel<Keep>, dim3((unsigned)ntiles), dim3(CC_BLOCK), 0, 0, keep, sc, count, tiles.get());
    hipLaunchKernelGGL(cc_scan_sums_kernel, dim3(1), dim3(SUMS_BLOCK), 0, 0, tiles.get(), ntiles, total_out);
    scatter((unsigned)ntiles);
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

void begin_call(double *t_call)
{
    for (int k = 0; k < PH_COUNT; ++k) phase_acc()[k] = 0.0;
    for (int k = 0; k < 8; ++k) kernel_ms()[k] = 0.0;
    *t_call = phase_now();
}

}  // namespace

extern "C" int gemhip_cc_labels(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, int32_t *labels_out, int32_t *n_components_out)
{
    double t_call;
    begin_call(&t_call);
    {
        PhaseScope ph(PH_HOST);
        GEMHIP_REQUIRE(labels_out && n_components_out, "cc_labels: NULL output");
        const int rc = validate("cc_labels", n, m, src, dst);
        if (rc) return rc;
    }
    Device D;
    const int rc = enqueue_labels(D, n, m, src, dst);
    if (rc) return rc;
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(D.ev.collect());
    {
        PhaseScope ph(PH_D2H);
        CcScalars sc;
        GEMHIP_CHECK(hipMemcpy(&sc, D.sc, sizeof sc, hipMemcpyDeviceToHost));
        GEMHIP_CHECK(hipMemcpy(labels_out, D.label, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        *n_components_out = sc.n_components;
    }
    phase_acc()[PH_TOTAL] = phase_now() - t_call;
    return GEMHIP_OK;
}

extern "C" int gemhip_lcc(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int64_t *n_out, int64_t *m_out,
                          int32_t *old_of_new, int32_t *new_of_old, int32_t *src_out, int32_t *dst_out, float *w_out, int32_t *n_components_out)
{
    double t_call;
    begin_call(&t_call);
    {
        PhaseScope ph(PH_HOST);
        GEMHIP_REQUIRE(n_out && m_out && old_of_new && new_of_old && n_components_out, "lcc: NULL output");
        GEMHIP_REQUIRE(m <= 0 || (src_out && dst_out), "lcc: NULL output");
        GEMHIP_REQUIRE((w == nullptr) == (w_out == nullptr), "lcc: w and w_out go together (both given or both NULL)");
        const int rc = validate("lcc", n, m, src, dst);
        if (rc) return rc;
    }
    Device D;
    DevBuf<float> dw;
    DevBuf<int32_t> d_new_of_old, d_old_of_new, d_src_out, d_dst_out, node_tiles, arc_tiles;
    DevBuf<uint32_t> d_w_out;
    if (w) {
        PhaseScope ph(PH_H2D);
        GEMHIP_CHECK(dw.upload(w, (size_t)m));
    }
    int rc = enqueue_labels(D, n, m, src, dst);
    if (rc) return rc;
    GEMHIP_CHECK(d_new_of_old.reserve((size_t)n));
    GEMHIP_CHECK(d_old_of_new.reserve((size_t)n));
    CcScalars *sc = D.sc.get();
    const KeepNode keep_node{D.label.get()};
    rc = enqueue_compaction(keep_node, sc, n, node_tiles, &sc->n_kept, [&](unsigned ntiles) {
        hipLaunchKernelGGL(cc_scatter_nodes_kernel, dim3(ntiles), dim3(CC_BLOCK), 0, 0, keep_node, sc, n, node_tiles.get(), d_new_of_old.get(), d_old_of_new.get());
    });
    if (rc) return rc;
    GEMHIP_CHECK(D.ev.mark());
    if (m > 0) {
        GEMHIP_CHECK(d_src_out.reserve((size_t)m));
        GEMHIP_CHECK(d_dst_out.reserve((size_t)m));
        if (w) GEMHIP_CHECK(d_w_out.reserve((size_t)m));
        const KeepArc keep_arc{D.src.get(), d_new_of_old.get()};
        rc = enqueue_compaction(keep_arc, sc, m, arc_tiles, &sc->m_kept, [&](unsigned ntiles) {
            hipLaunchKernelGGL(cc_scatter_arcs_kernel, dim3(ntiles), dim3(CC_BLOCK), 0, 0, keep_arc, m, D.dst.get(), (const uint32_t *)dw.get(), arc_tiles.get(),
                               d_src_out.get(), d_dst_out.get(), d_w_out.get());
        });
        if (rc) return rc;
    }
    GEMHIP_CHECK(D.ev.mark());
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(D.ev.collect());
    {
        PhaseScope ph(PH_D2H);
        CcScalars h;
        GEMHIP_CHECK(hipMemcpy(&h, D.sc, sizeof h, hipMemcpyDeviceToHost));
        if (h.n_kept < 1 || h.n_kept > n || h.m_kept < 0 || h.m_kept > m || (int64_t)(h.best >> 32) != h.n_kept)
            return fail(GEMHIP_E_HIP, "lcc: inconsistent device result (kept %d of %lld nodes, %d of %lld arcs, largest component %lld)", h.n_kept, (long long)n,
                        h.m_kept, (long long)m, (long long)(h.best >> 32));
        GEMHIP_CHECK(hipMemcpy(new_of_old, d_new_of_old, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
        GEMHIP_CHECK(hipMemcpy(old_of_new, d_old_of_new, (size_t)h.n_kept * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (h.m_kept > 0) {
            GEMHIP_CHECK(hipMemcpy(src_out, d_src_out, (size_t)h.m_kept * sizeof(int32_t), hipMemcpyDeviceToHost));
            GEMHIP_CHECK(hipMemcpy(dst_out, d_dst_out, (size_t)h.m_kept * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (w) GEMHIP_CHECK(hipMemcpy(w_out, d_w_out, (size_t)h.m_kept * sizeof(float), hipMemcpyDeviceToHost));
        }
        *n_out = h.n_kept; *m_out = h.m_kept; *n_components_out = h.n_components;
    }
    phase_acc()[PH_TOTAL] = phase_now() - t_call;
    return GEMHIP_OK;
}

extern "C" int gemhip_cc_last_kernel_ms(double *out)
{
    GEMHIP_REQUIRE(out != nullptr, "cc_last_kernel_ms: NULL");
    for (int k = 0; k < 8; ++k) out[k] = kernel_ms()[k];
    return GEMHIP_OK;
}
