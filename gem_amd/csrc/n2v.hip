// n2v.hip -- node2vec for MI355X (gfx950): transition tables, biased walks and vocabulary counts, and the one-shot gemhip_n2v_train.
//
// Replaces gem/embedding/node2vec.py:27-54, i.e. the subprocess call of the SNAP binary
// gem/c_exe/node2vec (`-i -o -d -l -r -k -e -p -q -v -dr -w`) and the text files around
// it.  Phases (symbols of the ELF) and their device equivalents:
//   PreprocessTransitionProbs/GetNodeAlias -> n2v_alias_rows_kernel (first-order Vose tables;
//        2nd-order bias by rejection sampling inside the walk, no sum(deg^2) tables)
//   SimulateWalk/AliasDrawInt             -> n2v_walk_kernel   (one lane = one walker)
//   LearnVocab                            -> n2v_vocab_kernel
//   InitUnigramTable                      -> host Vose in fp64 (O(n), once): sgns_plan.hip build_unigram_tables, uploaded by sgns_api.hip
//   InitPosEmb/InitNegEmb                 -> sgns_init_kernel (sgns_api.hip)
//   TrainModel (Hogwild over walks)       -> sgns_win_kernel / sgns_kernel (sgns.hpp; one wavefront = one walk), instantiated in
//        sgns_hogwild.hip, sgns_det.hip and sgns_part.hip (one bucket of the partitioned N-GPU schedule), launched by sgns_api.hip
// This file holds the handle's create / destroy, the alias, walk and count kernels and their accessors: it words refusals, moves data, and launches.
// What gemhip_n2v_create derives from the CSR is host arithmetic without a device (n2v_graph.hip); the handle itself is n2v_handle.hpp.
//
// All randomness is a counter-based Philox4x32-10 stream keyed by (seed, walk, position,
// purpose): results do not depend on scheduling, and the CPU oracle reproduces walks,
// counts and alias tables bit for bit.
#include "sgns.hpp"
#include "n2v_handle.hpp"
#include "n2v_graph.hpp"
#include <vector>
#include <cstdlib>
#include <algorithm>

using namespace gemhip;

namespace {
// Stateless stand-in for SNAP's NIdsV.Shuffle(): 4-round Feistel bijection, cycle-walked into [0,n).
__host__ __device__ __forceinline__ uint32_t perm_node(uint32_t j, uint32_t n, uint32_t hb, uint64_t key)
{
    const uint32_t mask = (1u << hb) - 1u;
    do {
        uint32_t L = j >> hb, R = j & mask;
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t k = (uint32_t)(key >> ((r & 1u) * 32)) + r * 0x9E3779B9u;
            const uint32_t t = L ^ (fmix32(R + k) & mask);
            L = R; R = t;
        }
        j = (L << hb) | R;
    } while (j >= n);
    return j;
}

// ------------------------------------------------------------------ alias tables
// GetNodeAlias (ELF @0x4115f0): one thread per CSR row, sequential Vose in fp32.  The two
// stacks share the row's segment of `work` (small grows up from 0, large down from N-1).
__global__ void n2v_alias_rows_kernel(int64_t n, const int64_t *__restrict__ row_ptr, const float *__restrict__ w,
                                      float *__restrict__ U, int32_t *__restrict__ K, int32_t *__restrict__ work_all)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int64_t a = row_ptr[v];
    const int32_t N = (int32_t)(row_ptr[v + 1] - a);
    if (N == 0 || N >= ALIAS_HUB_DEG) return;                  // (hub rows: n2v_alias_hub_kernel)
    const float *wt = w + a; float *Ur = U + a; int32_t *Kr = K + a; int32_t *work = work_all + a;
    float sum = 0.0f;
    for (int32_t i = 0; i < N; ++i) sum += wt[i];
    int32_t ns = 0, nl = 0;
    for (int32_t i = 0; i < N; ++i) {
        Kr[i] = 0;
        const float u = (wt[i] / sum) * (float)N;
        Ur[i] = u;
        if (u < 1.0f) work[ns++] = i; else work[N - 1 - nl++] = i;
    }
    while (ns > 0 && nl > 0) {
        const int32_t s = work[--ns];
        const int32_t l = work[N - nl]; --nl;
        Kr[s] = l;
        const float u = Ur[l] + Ur[s] - 1.0f;
        Ur[l] = u;
        if (u < 1.0f) work[ns++] = l; else work[N - 1 - nl++] = l;
    }
    while (ns > 0) Ur[work[--ns]] = 1.0f;
    while (nl > 0) { Ur[work[N - nl]] = 1.0f; --nl; }
}

// GetNodeAlias for HUB rows (N >= ALIAS_HUB_DEG): one workgroup per row, no N-step chain.  The stacks of GetNodeAlias are filled in index order and
// popped from the back, so smalls and larges are met in descending index order and the loop's outcome is closed form in two prefix sums -- D_j, the
// deficits of the first j smalls, and E_m, the excesses of the first m larges (both in stack order):
//   small s_j -> K = L_m, m = min{m : E_m >= D_{j-1}};   large L_m turns small at the first j with D_j > E_m: U = 1 + E_m - D_j, K = L_{m+1}
// (derivation and the proof by test against the sequential loop: oracle/n2v_oracle.c oracle_alias_build_hub, tests/test_oracle_n2v.py).  fp64, with
// the order of every sum FIXED exactly as the oracle fixes it -- chunks of 256 entries in stack order, sequential inside a chunk (one thread per
// chunk), chunk totals accumulated sequentially (thread 0), entry = chunk base + running sum -- so the table is the oracle's bit for bit whatever the
// block size.  scr: per row 2 N int32 (S, L) then 2 N double (D, E) then per-chunk {double d, e; int32 s, l}; a 94 115-neighbour R-MAT hub takes
// ~0.1 ms instead of a 94k-step dependent chain on one lane.
constexpr int ALIAS_CHUNK = 256;
__global__ __launch_bounds__(256) void n2v_alias_hub_kernel(const int32_t *__restrict__ hubs, const int64_t *__restrict__ hub_off, const int64_t *__restrict__ row_ptr,
                                                            const float *__restrict__ w, float *__restrict__ U, int32_t *__restrict__ K, unsigned char *__restrict__ scr_all)
{
#pragma clang fp contract(off)          // the oracle is built with -ffp-contract=off: `1.0 - (w / total) * N` must round the product first, here too
    const int32_t v = hubs[blockIdx.x];
    const int64_t a = row_ptr[v];
    const int32_t N = (int32_t)(row_ptr[v + 1] - a);
    const int32_t nch = (N + ALIAS_CHUNK - 1) / ALIAS_CHUNK;
    const float *wt = w + a; float *Ur = U + a; int32_t *Kr = K + a;
    // scratch segment of this row: hub_off counts entries; every entry owns 24 bytes, every chunk 24 more (chunks of row b start after all entries)
    unsigned char *scr = scr_all + (size_t)hub_off[blockIdx.x] * 24 + (size_t)(hub_off[blockIdx.x] / ALIAS_CHUNK + blockIdx.x) * 24;
    double *D = reinterpret_cast<double *>(scr), *E = D + N;
    int32_t *S = reinterpret_cast<int32_t *>(E + N), *L = S + N;
    double *cd = reinterpret_cast<double *>(scr + (size_t)N * 24), *ce = cd + nch;
    int32_t *cs = reinterpret_cast<int32_t *>(ce + nch), *cl = cs + nch;
    __shared__ double sh_total;
    __shared__ int32_t sh_ns, sh_nl;
    // total weight: chunk sums in INDEX order (into cd), accumulated sequentially
    for (int32_t c = threadIdx.x; c < nch; c += blockDim.x) {
        double t = 0.0;
        const int32_t i1 = (c + 1) * ALIAS_CHUNK < N ? (c + 1) * ALIAS_CHUNK : N;
        for (int32_t i = c * ALIAS_CHUNK; i < i1; ++i) t += (double)wt[i];
        cd[c] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int32_t c = 0; c < nch; ++c) t += cd[c]; sh_total = t; }
    __syncthreads();
    const double total = sh_total, dN = (double)N;
    // per chunk of the STACK order (r = 0 is the top of both stacks, i = N - 1 - r): deficit / excess sums and counts
    for (int32_t c = threadIdx.x; c < nch; c += blockDim.x) {
        double ds = 0.0, es = 0.0; int32_t ns = 0, nl = 0;
        const int32_t r1 = (c + 1) * ALIAS_CHUNK < N ? (c + 1) * ALIAS_CHUNK : N;
        for (int32_t r = c * ALIAS_CHUNK; r < r1; ++r) {
            const double u = ((double)wt[N - 1 - r] / total) * dN;
            if (u < 1.0) { ds += 1.0 - u; ++ns; } else { es += u - 1.0; ++nl; }
        }
        cd[c] = ds; ce[c] = es; cs[c] = ns; cl[c] = nl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                  // exclusive prefix over the chunks, sequential
        double bd = 0.0, be = 0.0; int32_t bs = 0, bl = 0;
        for (int32_t c = 0; c < nch; ++c) {
            const double ds = cd[c], es = ce[c]; const int32_t ns = cs[c], nl = cl[c];
            cd[c] = bd; ce[c] = be; cs[c] = bs; cl[c] = bl;
            bd += ds; be += es; bs += ns; bl += nl;
        }
        sh_ns = bs; sh_nl = bl;
    }
    __syncthreads();
    for (int32_t c = threadIdx.x; c < nch; c += blockDim.x) {
        double ds = 0.0, es = 0.0; int32_t ns = cs[c], nl = cl[c];
        const double bd = cd[c], be = ce[c];
        const int32_t r1 = (c + 1) * ALIAS_CHUNK < N ? (c + 1) * ALIAS_CHUNK : N;
        for (int32_t r = c * ALIAS_CHUNK; r < r1; ++r) {
            const int32_t i = N - 1 - r;
            const double u = ((double)wt[i] / total) * dN;
            Kr[i] = 0;
            if (u < 1.0) { ds += 1.0 - u; S[ns] = i; D[ns] = bd + ds; ++ns; Ur[i] = (float)u; }
            else { es += u - 1.0; L[nl] = i; E[nl] = be + es; ++nl; Ur[i] = 1.0f; }
        }
    }
    __threadfence_block();
    __syncthreads();
    const int32_t NS = sh_ns, NL = sh_nl;
    for (int32_t j = threadIdx.x; j < NS; j += blockDim.x) {  // smalls: first m with E[m] >= D[j-1]
        const double dp = j ? D[j - 1] : 0.0;
        int32_t lo = 0, hi = NL;
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (E[mid] >= dp) hi = mid; else lo = mid + 1; }
        if (lo < NL) Kr[S[j]] = L[lo]; else Ur[S[j]] = 1.0f;
    }
    for (int32_t m = threadIdx.x; m < NL; m += blockDim.x) {  // larges: first j with D[j] > E[m]
        const double em = E[m];
        int32_t lo = 0, hi = NS;
        while (lo < hi) { const int32_t mid = (lo + hi) >> 1; if (D[mid] > em) hi = mid; else lo = mid + 1; }
        if (lo < NS && m + 1 < NL) { Ur[L[m]] = (float)(1.0 + em - D[lo]); Kr[L[m]] = L[m + 1]; }
    }
}

// ------------------------------------------------------------------------- walks
__device__ __forceinline__ bool has_edge_sorted(const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col, int32_t t, int32_t x)
{
    int64_t lo = row_ptr[t];
    const int64_t end = row_ptr[t + 1];
    int64_t hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (col[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < end && col[lo] == x;
}

// SimulateWalk (ELF @0x411a00).  One lane per walk; tokens are buffered 16 at a time in
// registers so each lane writes 64 contiguous bytes (dwordx4 stores) instead of 4-byte scatters.
template <bool SECOND, bool WEIGHTED>
__global__ __launch_bounds__(256) void n2v_walk_kernel(int64_t n, int64_t m, const int32_t *__restrict__ start, uint32_t hb, const int64_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ col, const float *__restrict__ U,
                                                       const int32_t *__restrict__ K, float ip, float iq, float amax,
                                                       int32_t walk_len, uint64_t seed, int32_t flags, int64_t walk_begin,
                                                       int64_t count, int32_t *__restrict__ walks)
{
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= count) return;
    const int64_t wid = walk_begin + tid;
    const uint32_t round = (uint32_t)(wid / m), j = (uint32_t)(wid % m);
    int32_t cur = start[perm_node(j, (uint32_t)m, hb, seed ^ ((uint64_t)(round + 1) * 0x9E3779B97F4A7C15ull))];
    int32_t prev = -1;
    const int32_t pad = (flags & 1) ? 0 : -1;
    const bool uniform_first = (flags & 8) != 0;
    bool alive = true;
    int32_t *out = walks + tid * walk_len;
    const bool vec_ok = (walk_len & 3) == 0;

    for (int32_t base = 0; base < walk_len; base += 16) {
        int32_t buf[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int32_t len = base + k;       // number of tokens already emitted == index of this token
            int32_t tok = pad;
            if (len == 0) tok = cur;
            else if (len < walk_len && alive) {
                const int64_t a = row_ptr[cur];
                const uint32_t deg = (uint32_t)(row_ptr[cur + 1] - a);
                if (deg == 0) alive = false;
                else {
                    int32_t nxt = -1;
                    for (uint32_t trial = 0;; ++trial) {
                        const u32x4 r = philox4x32_10(seed, (uint32_t)wid, (uint32_t)((uint64_t)wid >> 32), (uint32_t)len,
                                                      (uint32_t)TAG_WALK | (trial << 8));
                        uint32_t slot = mulhi_range(r.x, deg);
                        if (WEIGHTED && !(len == 1 && uniform_first)) {
                            if (!(u01(r.y) < U[a + slot])) slot = (uint32_t)K[a + slot];
                        }
                        const int32_t x = col[a + slot];
                        if (!SECOND || len == 1) { nxt = x; break; }
                        const float alpha = (x == prev) ? ip : (has_edge_sorted(row_ptr, col, prev, x) ? 1.0f : iq);
                        if (u01(r.z) * amax < alpha || trial >= 4095u) { nxt = x; break; }
                    }
                    prev = cur; cur = nxt; tok = nxt;
                }
            }
            buf[k] = tok;
        }
        if (vec_ok) {
#pragma unroll
            for (int k = 0; k < 16; k += 4)
                if (base + k < walk_len) *reinterpret_cast<int4 *>(out + base + k) = make_int4(buf[k], buf[k + 1], buf[k + 2], buf[k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (base + k < walk_len) out[base + k] = buf[k];
        }
    }
}

// LearnVocab (ELF @0x40d560): token histogram.
__global__ void n2v_vocab_kernel(const int32_t *__restrict__ walks, int64_t ntokens, int32_t *__restrict__ counts)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ntokens; i += stride) {
        const int32_t t = walks[i];
        if (t >= 0) atomicAdd(&counts[t], 1);
    }
}

uint32_t half_bits(uint64_t n)
{
    uint32_t bits = 1;
    while (((uint64_t)1 << bits) < n) ++bits;
    return (bits + 1) / 2;
}

}  // namespace

// ------------------------------------------------------------------- host API
extern "C" int gemhip_n2v_create(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w,
                                 gemhip_n2v_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "n2v_create: out is NULL");
    *out = nullptr;
    // everything that needs no device: validation, rows sorted with their weights following, start nodes, hub rows (n2v_graph.hip)
    const double t_host0 = phase_now();
    N2vGraph g;
    const N2vGraphError bad = prepare_n2v_graph(n, nnz, row_ptr, col, w, g);
    using E = N2vGraphError;
    GEMHIP_REQUIRE(bad.kind != E::N_OUT_OF_RANGE, "n2v_create: n=%lld out of range", (long long)n);
    GEMHIP_REQUIRE(bad.kind != E::BAD_ARRAYS, "n2v_create: bad CSR arrays");
    GEMHIP_REQUIRE(bad.kind != E::ROW_PTR_FIRST && bad.kind != E::ROW_PTR_LAST, "n2v_create: row_ptr[0]=%lld row_ptr[n]=%lld nnz=%lld",
                   (long long)row_ptr[0], (long long)row_ptr[n], (long long)nnz);
    GEMHIP_REQUIRE(bad.kind != E::ROW_PTR_NOT_MONOTONE, "n2v_create: row_ptr not monotone at row %lld", (long long)bad.index);
    GEMHIP_REQUIRE(bad.kind != E::COLUMN_OUT_OF_RANGE, "n2v_create: column %d outside [0,%lld)", bad.column, (long long)n);
    GEMHIP_REQUIRE(bad.kind != E::NON_POSITIVE_WEIGHT, "n2v_create: non-positive weight at edge %lld", (long long)bad.index);
    auto *h = new gemhip_n2v();
    h->n = n; h->nnz = nnz; h->uniform_rows = g.uniform; h->m_start = (int64_t)g.start.size();
    h->hub_rows = std::move(g.hub_rows); h->hub_off = std::move(g.hub_off);
    // A/B knobs: read ONCE, here (the launch path reads no environment); the setters of sgns_api.hip override them per handle
    h->kn = sgns_knobs_from_env([](const char *name) -> const char * { return getenv(name); });
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail(GEMHIP_E_HIP, "n2v_create: no HIP device"); }
    phase_acc()[PH_HOST] += phase_now() - t_host0;
    PhaseScope ph_up(PH_H2D);
    hipError_t e = h->d_row_ptr.upload(row_ptr, n + 1);
    if (e == hipSuccess) e = h->d_col.upload(g.col.data(), nnz);
    if (e == hipSuccess && !g.uniform) e = h->d_w.upload(g.w.data(), nnz);
    if (e == hipSuccess) e = h->d_start.upload(g.start.data(), g.start.size());
    if (e == hipSuccess) e = h->counts_own.reserve(n);
    h->d_counts = h->counts_own;
    if (e == hipSuccess) e = h->d_pairs.reserve(1);
    if (e == hipSuccess) e = hipMemset(h->d_pairs, 0, sizeof(unsigned long long));
    if (e != hipSuccess) { gemhip_n2v_destroy(h); return fail(GEMHIP_E_HIP, "n2v_create: device upload failed: %s", hipGetErrorString(e)); }
    *out = h;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_destroy(gemhip_n2v_t h)
{
    if (!h) return GEMHIP_OK;
    delete h;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_build_alias(gemhip_n2v_t h, void *stream)
{
    GEMHIP_REQUIRE(h, "n2v_build_alias: NULL handle");
    if (h->uniform_rows || h->d_U) return GEMHIP_OK;
    // built in locals and handed to the handle only when complete: an error exit leaves the handle without tables (the next call builds again)
    DevBuf<float> U; DevBuf<int32_t> K, work, d_hubs; DevBuf<int64_t> d_hoff; DevBuf<unsigned char> d_scr;
    GEMHIP_CHECK(U.reserve(h->nnz));
    GEMHIP_CHECK(K.reserve(h->nnz));
    GEMHIP_CHECK(work.reserve(h->nnz));
    hipLaunchKernelGGL(n2v_alias_rows_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->n,
                       h->d_row_ptr, h->d_w, U, K, work);
    GEMHIP_CHECK(hipGetLastError());
    if (!h->hub_rows.empty()) {                        // hub rows: a workgroup each (the one-lane kernel skipped them)
        const size_t nh = h->hub_rows.size();
        const size_t entries = (size_t)h->hub_off.back();
        const size_t scr_bytes = entries * 24 + (entries / ALIAS_CHUNK + nh + 1) * 24;
        GEMHIP_CHECK(d_hubs.reserve(nh));
        GEMHIP_CHECK(d_hoff.reserve(nh + 1));
        GEMHIP_CHECK(d_scr.reserve(scr_bytes));
        GEMHIP_CHECK(hipMemcpyAsync(d_hubs, h->hub_rows.data(), nh * sizeof(int32_t), hipMemcpyHostToDevice, (hipStream_t)stream));
        GEMHIP_CHECK(hipMemcpyAsync(d_hoff, h->hub_off.data(), (nh + 1) * sizeof(int64_t), hipMemcpyHostToDevice, (hipStream_t)stream));
        hipLaunchKernelGGL(n2v_alias_hub_kernel, dim3((unsigned)nh), dim3(256), 0, (hipStream_t)stream, d_hubs, d_hoff, h->d_row_ptr, h->d_w, U, K, d_scr);
        GEMHIP_CHECK(hipGetLastError());
    }
    GEMHIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    h->d_U = std::move(U); h->d_K = std::move(K);
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_get_alias(gemhip_n2v_t h, float *U_host, int32_t *K_host, int32_t *col_sorted_host)
{
    GEMHIP_REQUIRE(h, "n2v_get_alias: NULL handle");
    if (col_sorted_host && h->nnz) GEMHIP_CHECK(hipMemcpy(col_sorted_host, h->d_col, h->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (h->uniform_rows) return 1;          // no tables: rows are uniform
    GEMHIP_REQUIRE(h->d_U, "n2v_get_alias: build_alias not called");
    if (U_host) GEMHIP_CHECK(hipMemcpy(U_host, h->d_U, h->nnz * sizeof(float), hipMemcpyDeviceToHost));
    if (K_host) GEMHIP_CHECK(hipMemcpy(K_host, h->d_K, h->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

static int ensure_walk_buffer(gemhip_n2v_t h, int64_t nwalks, int32_t walk_len)
{
    const int64_t need = nwalks * walk_len;
    if ((size_t)need > h->d_walks.capacity()) GEMHIP_CHECK(h->d_walks.reserve(need));          // (no walks asked for and none held: stays empty)
    h->nwalks = nwalks; h->walk_len = walk_len;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_walks(gemhip_n2v_t h, float p, float q, int32_t num_walks, int32_t walk_len, uint64_t seed,
                                int32_t flags, int64_t walk_begin, int64_t walk_end, void *stream)
{
    GEMHIP_REQUIRE(h, "n2v_walks: NULL handle");
    GEMHIP_REQUIRE(p > 0.f && q > 0.f, "n2v_walks: p=%g q=%g must be > 0", (double)p, (double)q);
    GEMHIP_REQUIRE(num_walks >= 1 && walk_len >= 1 && walk_len < 65536, "n2v_walks: num_walks=%d walk_len=%d", num_walks, walk_len);
    const int64_t total = h->m_start * (int64_t)num_walks;
    GEMHIP_REQUIRE(0 <= walk_begin && walk_begin <= walk_end && walk_end <= total, "n2v_walks: bad walk range [%lld,%lld) of %lld",
                   (long long)walk_begin, (long long)walk_end, (long long)total);
    if (!h->uniform_rows && !h->d_U) { if (int rc = gemhip_n2v_build_alias(h, stream)) return rc; }
    const int64_t count = walk_end - walk_begin;
    if (int rc = ensure_walk_buffer(h, count, walk_len)) return rc;
    h->walk_id_offset = walk_begin;
    corpus_changed(h);
    if (count == 0) return GEMHIP_OK;
    const bool second = !(p == 1.0f && q == 1.0f);
    const float ip = 1.0f / p, iq = 1.0f / q;
    const float amax = std::max(1.0f, std::max(ip, iq));
    const dim3 grid((unsigned)((count + 255) / 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t hb = half_bits((uint64_t)h->m_start);
#define N2V_WALK(S, W) hipLaunchKernelGGL((n2v_walk_kernel<S, W>), grid, block, 0, s, h->n, h->m_start, h->d_start, hb, h->d_row_ptr, h->d_col, h->d_U, h->d_K, ip, \
                                          iq, amax, walk_len, seed, flags, walk_begin, count, h->d_walks)
    if (second) { if (h->uniform_rows) N2V_WALK(true, false); else N2V_WALK(true, true); }
    else        { if (h->uniform_rows) N2V_WALK(false, false); else N2V_WALK(false, true); }
#undef N2V_WALK
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_start_nodes(gemhip_n2v_t h, int64_t *m)
{
    GEMHIP_REQUIRE(h && m, "n2v_start_nodes: NULL argument");
    *m = h->m_start;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_set_walks(gemhip_n2v_t h, const int32_t *walks_host, int64_t nwalks, int32_t walk_len, int64_t walk_id_offset)
{
    GEMHIP_REQUIRE(h && walks_host && nwalks >= 0 && walk_len >= 1 && walk_len < 65536, "n2v_set_walks: bad arguments");
    if (int rc = ensure_walk_buffer(h, nwalks, walk_len)) return rc;
    h->walk_id_offset = walk_id_offset;
    corpus_changed(h);
    if (nwalks) GEMHIP_CHECK(hipMemcpy(h->d_walks, walks_host, nwalks * walk_len * sizeof(int32_t), hipMemcpyHostToDevice));
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_get_walks(gemhip_n2v_t h, int32_t *walks_host)
{
    GEMHIP_REQUIRE(h && walks_host, "n2v_get_walks: NULL argument");
    GEMHIP_CHECK(hipDeviceSynchronize());
    if (h->nwalks) GEMHIP_CHECK(hipMemcpy(walks_host, h->d_walks, h->nwalks * h->walk_len * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_walks_ptr(gemhip_n2v_t h, void **d_walks, int64_t *nwalks, int32_t *walk_len)
{
    GEMHIP_REQUIRE(h && d_walks, "n2v_walks_ptr: NULL argument");
    *d_walks = h->d_walks;
    if (nwalks) *nwalks = h->nwalks;
    if (walk_len) *walk_len = h->walk_len;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_vocab(gemhip_n2v_t h, void *stream)
{
    GEMHIP_REQUIRE(h, "n2v_vocab: NULL handle");
    hipStream_t s = (hipStream_t)stream;
    GEMHIP_CHECK(hipMemsetAsync(h->d_counts, 0, h->n * sizeof(int32_t), s));
    const int64_t ntok = h->nwalks * h->walk_len;
    if (ntok) {
        const int64_t blocks = std::min<int64_t>((ntok + 255) / 256, 256 * 16);
        hipLaunchKernelGGL(n2v_vocab_kernel, dim3((unsigned)blocks), dim3(256), 0, s, h->d_walks, ntok, h->d_counts);
        GEMHIP_CHECK(hipGetLastError());
    }
    corpus_changed(h);
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_bind_counts(gemhip_n2v_t h, void *d_counts)
{
    GEMHIP_REQUIRE(h && d_counts, "n2v_bind_counts: NULL argument");
    h->counts_own.reset();
    h->d_counts = (int32_t *)d_counts; corpus_changed(h);
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_counts_ptr(gemhip_n2v_t h, void **d_counts)
{
    GEMHIP_REQUIRE(h && d_counts, "n2v_counts_ptr: NULL argument");
    *d_counts = h->d_counts;
    return GEMHIP_OK;
}

// D2D copy of local walks [walk_lo, walk_hi) into a caller-owned device buffer (e.g. a torch tensor that an all-gather then assembles the corpus from)
extern "C" int gemhip_n2v_copy_walks(gemhip_n2v_t h, int64_t walk_lo, int64_t walk_hi, void *d_dst, void *stream)
{
    GEMHIP_REQUIRE(h && d_dst && 0 <= walk_lo && walk_lo <= walk_hi && walk_hi <= h->nwalks, "n2v_copy_walks: bad arguments");
    if (walk_hi > walk_lo)
        GEMHIP_CHECK(hipMemcpyAsync(d_dst, h->d_walks + walk_lo * h->walk_len, (size_t)(walk_hi - walk_lo) * h->walk_len * sizeof(int32_t), hipMemcpyDeviceToDevice,
                                    (hipStream_t)stream));
    return GEMHIP_OK;
}

// One-shot drop-in for `node2vec -i -o -d -l -r -k -e -p -q -dr -w` (node2vec.py:34-53).
extern "C" int gemhip_n2v_train(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t d,
                                int32_t walk_len, int32_t num_walks, int32_t window, int32_t epochs, float p, float q,
                                uint64_t seed, int32_t flags, float *X_out, double *stats)
{
    GEMHIP_REQUIRE(X_out != nullptr, "n2v_train: X_out is NULL");
    for (int k = 0; k < PH_COUNT; ++k) phase_acc()[k] = 0.0;
    const double t_call = phase_now();
    gemhip_n2v_t h = nullptr;
    int rc = gemhip_n2v_create(n, nnz, row_ptr, col, w, &h);
    if (rc) return rc;
    EventMarks<4> ev;
    if (ev.create() != hipSuccess) rc = fail(GEMHIP_E_HIP, "n2v_train: hipEventCreate");
    const int64_t nwalks = h->m_start * (int64_t)num_walks;
    if (!rc) { (void)ev.mark(0); rc = gemhip_n2v_walks(h, p, q, num_walks, walk_len, seed, flags, 0, nwalks, nullptr); }
    if (!rc) rc = gemhip_n2v_vocab(h, nullptr);
    if (!rc) { (void)ev.mark(1); rc = (flags & GEMHIP_N2V_VOCAB_ORDER) ? gemhip_n2v_build_unigram_vocab_order(h, flags, nullptr, nullptr, nullptr, nullptr)
                                                                         : gemhip_n2v_build_unigram(h, nullptr, nullptr, nullptr); }
    if (!rc) rc = gemhip_sgns_init(h, d, seed, nullptr, nullptr);
    if (!rc) (void)ev.mark(2);
    for (int ep = 0; !rc && ep < epochs; ++ep)
        rc = gemhip_sgns_train(h, window, SGNS_NEG, 0.025f, epochs, ep, 0, nwalks, nwalks * walk_len, (int64_t)ep * nwalks * walk_len,
                               seed, flags, nullptr);
    if (!rc) { (void)ev.mark(3); rc = gemhip_sgns_get_tables(h, X_out, nullptr); }
    if (!rc) {     // kernel seconds of the call (HIP events): walks + vocabulary, then table init + SGNS
        double a = 0.0, b = 0.0;
        (void)ev.ms(0, 1, &a);
        (void)ev.ms(2, 3, &b);
        if (stats) { stats[0] = a * 1e-3; stats[1] = b * 1e-3; stats[2] = (double)nwalks * walk_len; stats[3] = h->uniform_rows ? 1.0 : 0.0; }
        phase_acc()[PH_KERNELS] = (a + b) * 1e-3;
    }
    gemhip_n2v_destroy(h);
    phase_acc()[PH_TOTAL] = phase_now() - t_call;
    return rc;
}
