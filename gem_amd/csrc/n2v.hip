// n2v.hip -- node2vec for MI355X (gfx950): transition tables, biased walks, vocabulary
// counts, and skip-gram with negative sampling (SGNS).
//
// Replaces gem/embedding/node2vec.py:27-54, i.e. the subprocess call of the SNAP binary
// gem/c_exe/node2vec (`-i -o -d -l -r -k -e -p -q -v -dr -w`) and the text files around
// it.  Phases (symbols of the ELF) and their device equivalents:
//   PreprocessTransitionProbs/GetNodeAlias -> n2v_alias_rows_kernel (first-order Vose tables;
//        2nd-order bias by rejection sampling inside the walk, no sum(deg^2) tables)
//   SimulateWalk/AliasDrawInt             -> n2v_walk_kernel   (one lane = one walker)
//   LearnVocab                            -> n2v_vocab_kernel
//   InitUnigramTable                      -> host Vose in fp64 (O(n), once): sgns_plan.hip build_unigram_tables
//   InitPosEmb/InitNegEmb                 -> sgns_init_kernel
//   TrainModel (Hogwild over walks)       -> sgns_win_kernel / sgns_kernel (sgns.hpp; one wavefront = one walk), instantiated in
//        sgns_hogwild.hip, sgns_det.hip and sgns_part.hip (one bucket of the partitioned N-GPU schedule)
// This file holds the kernels of everything but TrainModel and the C ABI: it validates, moves data, and launches.  What a launch looks like and what
// the unigram tables contain is host arithmetic without a device: sgns_plan.hip (VocabStats, SgnsKnobs, plan_sgns_launch, bucket_knobs, UnigramTables).
//
// All randomness is a counter-based Philox4x32-10 stream keyed by (seed, walk, position,
// purpose): results do not depend on scheduling, and the CPU oracle reproduces walks,
// counts and alias tables bit for bit.
#include "sgns.hpp"
#include <hipcub/hipcub.hpp>
#include <vector>
#include <cstring>
#include <cmath>
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
}  // namespace

struct gemhip_n2v {
    int64_t n = 0, nnz = 0;
    int device = 0;
    bool uniform_rows = true;         // every row has equal weights -> no alias tables needed
    DevBuf<int64_t> d_row_ptr;
    DevBuf<int32_t> d_col;            // columns sorted inside each row
    // walk start nodes: the nodes that occur in the edge list (the reference binary only knows those; an isolated node
    // never reaches it).  start[0..m_start) ascending; walk id r*m_start + j starts at start[perm_r(j)]
    int64_t m_start = 0;
    DevBuf<int32_t> d_start;
    DevBuf<float> d_w;
    std::vector<int32_t> hub_rows;    // rows with at least ALIAS_HUB_DEG neighbours (n2v_alias_hub_kernel builds their tables: a workgroup per row)
    std::vector<int64_t> hub_off;     // ... and the offset of each one's scratch segment (prefix sum of their degrees)
    DevBuf<float> d_U;                // first-order alias tables (per-row segments)
    DevBuf<int32_t> d_K;
    // walks
    DevBuf<int32_t> d_walks;          // capacity in tokens
    int64_t nwalks = 0;               // local walks held
    int32_t walk_len = 0;
    int64_t walk_id_offset = 0;       // global id of local walk 0
    // vocabulary / unigram
    int32_t *d_counts = nullptr;      // what the kernels read: counts_own's block, or the caller's (gemhip_n2v_bind_counts)
    DevBuf<int32_t> counts_own;       // empty while the counts are borrowed
    DevBuf<float> d_UT;
    DevBuf<int32_t> d_KT;
    DevBuf<uint2> d_UK;                // {bits of UT[i], KT[i]} interleaved: one 8-byte gather instead of two 4-byte gathers
    bool unigram_ready = false;
    // slot tables of the window kernels (SgnsArgs::SK): {X, UT[X], KT[X]} by SLOT, built on the device from the tables above on the first launch
    // after a table build, once per RndUnigramInt-quirk setting (sk_state / skp_state: -1 stale, else the quirk bit they were built for)
    DevBuf<uint4> d_SK; int sk_state = -1;
    DevBuf<uint4> d_SKp; int skp_state = -1;
    // vocabulary-order layout (gemhip_n2v_build_unigram_vocab_order): the slot table of RndUnigramInt, and how many slots it has
    DevBuf<int32_t> d_KTslot; int64_t n_vocab = 0; bool vocab_order = false;
    DevBuf<unsigned long long> d_first;      // first token index of every node (scratch of that builder)
    // embeddings
    int32_t d = 0;
    float *SynPos = nullptr, *SynNeg = nullptr;   // what the kernels train: syn_own's blocks, or the caller's tables (gemhip_sgns_init)
    DevBuf<float> syn_own[2];         // empty while the tables are borrowed
    SgnsKnobs kn;                     // launch knobs (setters below; environment overrides read once in gemhip_n2v_create)
    DevBuf<int32_t> d_hotkey, d_wcount; DevBuf<unsigned int> d_nlocal; int hotkey_state = 0; int64_t n_local_hot = 0;   // LOCALLY HOT ROWS (build_hotkey)
    SgnsLaunchPlan last_plan;         // what the last gemhip_sgns_train / _train_part on this handle actually launched (gemhip_sgns_last_launch)
    int32_t last_fresh = 0;
    VocabStats vs;                    // vocabulary statistics (gemhip_n2v_build_unigram*): how concentrated the row traffic is -> plan_sgns_launch
    DevBuf<float> d_dummy;       // sgns_win_kernel: one scratch row per wavefront
    DevBuf<float> d_scratch;     // sgns_win_kernel<PART>: the window rows as loaded, 2R+1 rows per wavefront
    DevBuf<unsigned long long> d_pairs;      // (centre,context) pairs trained so far
    // per-partition unigram tables (multi-GPU episode schedule): partition p = {v : v % parts == p}, local index v / parts
    int32_t parts = 0;
    DevBuf<float> d_UTp; DevBuf<int32_t> d_KTp;
    DevBuf<uint2> d_UKp;                     // {bits of UTp[i], KTp[i]} interleaved (sgns_win_kernel<PART>)
    // ... in the binary's layout (gemhip_n2v_build_unigram_parts_vocab_order): per partition the slot table of RndUnigramInt in LOCAL indices
    // (d_KTslotp[part_off[p] + slot]) and its number of slots (the partition's nodes that occur); the alias arrays above are then indexed by local row
    DevBuf<int32_t> d_KTslotp; std::vector<int64_t> part_slots; bool parts_vocab_order = false;
    std::vector<int64_t> part_off;           // table p occupies [part_off[p], part_off[p+1])
    std::vector<VocabStats> vs_part;         // vocabulary statistics of each partition's rows (launch rule of gemhip_sgns_train_part)
};

namespace {

// ------------------------------------------------------------------ alias tables
constexpr int ALIAS_HUB_DEG = 2048;      // rows from this many neighbours on take n2v_alias_hub_kernel (oracle: ORACLE_ALIAS_HUB_DEG)
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

// LOCALLY HOT ROWS (round 6).  wcount[v] = number of walks that CONTAIN v (one wavefront per walk: a token counts at its first occurrence in the walk).
// A node whose tokens are packed into few walks -- count[v] / wcount[v] occurrences per walk that touches it -- sits in that walk's LDS window for the
// whole walk, not for 2R+1 centres: the two nodes of an isolated edge make up ALL 80 tokens of each of their 20 walks.  Two wavefronts that train two of
// those walks at the same time each apply a whole walk's worth of updates (~800 pair steps per row) to the same base and both deltas are added: the pair
// ends with a norm 14 % above its peers' (measured, R-MAT scale 17 at 1 536 wavefronts: profiles/r06_canaries_rmat17.jsonl) and, because the nodes of
// such components are nearly collinear (cosine 0.93; they are only ever pushed away from the same hub rows), outranks the true neighbour of dozens of
// them -- the heavy tail of the power-law "Hogwild bias" (each event costs 2-5 % of the graph's MAP; its probability grows with the width).
__global__ __launch_bounds__(64) void n2v_walk_presence_kernel(const int32_t *__restrict__ walks, int64_t nwalks, int32_t walk_len, int32_t *__restrict__ wcount)
{
    extern __shared__ int32_t tokp[];
    const int lane = threadIdx.x;
    for (int64_t wl = blockIdx.x; wl < nwalks; wl += gridDim.x) {
        const int32_t *walk = walks + wl * walk_len;
        for (int k = lane; k < walk_len; k += WAVE) tokp[k] = walk[k];
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < walk_len; k += WAVE) {
            const int32_t v = tokp[k];
            bool first = v >= 0;
            for (int q = 0; q < k && first; ++q) first = tokp[q] != v;
            if (first) atomicAdd(&wcount[v], 1);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// hotkey[v] = INT32_MAX for a locally hot node (count >= per_walk x walks containing it), else its token count: what the SGNS kernels compare with hot_thr
__global__ void n2v_hotkey_kernel(int64_t n, const int32_t *__restrict__ counts, const int32_t *__restrict__ wcount, int32_t per_walk, int32_t *__restrict__ hotkey,
                                  unsigned int *__restrict__ nlocal)
{
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const int32_t c = counts[v], w = wcount[v];
    const bool loc = w > 0 && (int64_t)c >= (int64_t)per_walk * w;
    hotkey[v] = loc ? INT32_MAX : c;
    if (loc) atomicAdd(nlocal, 1u);
}

// -------------------------------------------------------------------------- SGNS
// InitPosEmb (ELF @0x40e270): (U(0,1)-0.5)/d ; InitNegEmb: zeros.
// first[v] = index of the first token equal to v (LearnVocab @0x40d560 renames the tokens 0..N-1 in that order)
__global__ void n2v_first_token_kernel(const int32_t *__restrict__ walks, int64_t ntokens, unsigned long long *__restrict__ first)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < ntokens; t += stride) {
        const int32_t v = walks[t];
        if (v >= 0 && first[v] > (unsigned long long)t) atomicMin(&first[v], (unsigned long long)t);
    }
}

__global__ void iota_kernel(int32_t *p, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = (int32_t)i;
}

// SgnsArgs::SK.  RndUnigramInt draws slot = floor(u n), X = KT[slot] (quirk) or slot, then reads {UTable[X], KTable[X]}: the second gather depends on
// the first.  SK[slot] = {X, bits of UTable[X], KTable[X], 0} answers both with one 16-byte read (same values: the draws are unchanged bit for bit).
__global__ void n2v_slot_table_kernel(int64_t nslots, const int32_t *__restrict__ KT, const uint2 *__restrict__ UK, int quirk, uint4 *__restrict__ SK)
{
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int32_t X = quirk ? KT[s] : (int32_t)s;
    const uint2 uk = UK[X];
    SK[s] = make_uint4((uint32_t)X, uk.x, uk.y, 0u);
}

__global__ void sgns_init_kernel(float *SynPos, float *SynNeg, int64_t total, int32_t d, uint64_t seed)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t * 4 >= total) return;
    const u32x4 r = philox4x32_10(seed, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), 0u, (uint32_t)TAG_INIT);
    const uint32_t v[4] = {r.x, r.y, r.z, r.w};
    for (int k = 0; k < 4; ++k)
        if (t * 4 + k < total) {
            SynPos[t * 4 + k] = (u01(v[k]) - 0.5f) / (float)d;
            SynNeg[t * 4 + k] = 0.0f;
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
    GEMHIP_REQUIRE(n > 0 && n < (int64_t)0x7fffffff, "n2v_create: n=%lld out of range", (long long)n);
    GEMHIP_REQUIRE(nnz >= 0 && row_ptr && (nnz == 0 || col), "n2v_create: bad CSR arrays");
    GEMHIP_REQUIRE(row_ptr[0] == 0 && row_ptr[n] == nnz, "n2v_create: row_ptr[0]=%lld row_ptr[n]=%lld nnz=%lld",
                   (long long)row_ptr[0], (long long)row_ptr[n], (long long)nnz);
    // sort columns inside each row (needed by the has_edge test of the 2nd-order walk); weights follow
    const double t_host0 = phase_now();
    std::vector<int32_t> c(col, col + nnz);
    std::vector<float> ww;
    if (w) ww.assign(w, w + nnz);
    bool uniform = true;
    std::vector<std::pair<int32_t, float>> tmp;
    for (int64_t v = 0; v < n; ++v) {
        const int64_t a = row_ptr[v], b = row_ptr[v + 1];
        GEMHIP_REQUIRE(a <= b && b <= nnz, "n2v_create: row_ptr not monotone at row %lld", (long long)v);
        bool sorted = true;
        for (int64_t e = a; e < b; ++e) {
            GEMHIP_REQUIRE(c[e] >= 0 && c[e] < n, "n2v_create: column %d outside [0,%lld)", c[e], (long long)n);
            if (e > a && c[e] < c[e - 1]) sorted = false;
            if (w && w[e] != w[a]) uniform = false;
            if (w) GEMHIP_REQUIRE(w[e] > 0.f, "n2v_create: non-positive weight at edge %lld", (long long)e);
        }
        if (!sorted) {
            tmp.clear();
            for (int64_t e = a; e < b; ++e) tmp.emplace_back(c[e], w ? ww[e] : 1.f);
            std::stable_sort(tmp.begin(), tmp.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
            for (int64_t e = a; e < b; ++e) { c[e] = tmp[e - a].first; if (w) ww[e] = tmp[e - a].second; }
        }
    }
    std::vector<int32_t> start;
    {
        std::vector<char> present(n, 0);
        for (int64_t v = 0; v < n; ++v)
            if (row_ptr[v + 1] > row_ptr[v]) present[v] = 1;
        for (int64_t e = 0; e < nnz; ++e) present[c[e]] = 1;
        for (int64_t v = 0; v < n; ++v) if (present[v]) start.push_back((int32_t)v);
    }
    auto *h = new gemhip_n2v();
    h->n = n; h->nnz = nnz; h->uniform_rows = uniform; h->m_start = (int64_t)start.size();
    if (!uniform) {
        h->hub_off.push_back(0);
        for (int64_t v = 0; v < n; ++v)
            if (row_ptr[v + 1] - row_ptr[v] >= ALIAS_HUB_DEG) { h->hub_rows.push_back((int32_t)v); h->hub_off.push_back(h->hub_off.back() + (row_ptr[v + 1] - row_ptr[v])); }
    }
    // A/B knobs: read ONCE, here (the launch path reads no environment); the setters below override them per handle
    if (const char *e = getenv("GEMHIP_SGNS_MAX_WAVES")) h->kn.max_waves = std::max(0, atoi(e));
    if (const char *e = getenv("GEMHIP_SGNS_CACHE_R")) h->kn.cache_radius = std::min(31, std::max(-1, atoi(e)));
    if (const char *e = getenv("GEMHIP_SGNS_CACHE_DELTA")) h->kn.cache_delta = std::min(1, std::max(-1, atoi(e)));
    if (const char *e = getenv("GEMHIP_SGNS_PREFETCH")) h->kn.prefetch = std::min(2, std::max(1, atoi(e)));
    if (const char *e = getenv("GEMHIP_SGNS_RELOAD")) h->kn.reload = atoi(e) != 0;
    if (const char *e = getenv("GEMHIP_SGNS_HOT_COUNT")) h->kn.hot_count = std::max(-1, atoi(e));
    if (const char *e = getenv("GEMHIP_SGNS_LOCAL_HOT")) h->kn.local_hot = std::max(0, atoi(e));
    if (const char *e = getenv("GEMHIP_SGNS_FRESH")) h->kn.fresh = atoi(e) & 7;
    if (const char *e = getenv("GEMHIP_SGNS_NEG_COUNT")) h->kn.neg_count = std::max(0, atoi(e));
    if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail(GEMHIP_E_HIP, "n2v_create: no HIP device"); }
    phase_acc()[PH_HOST] += phase_now() - t_host0;
    PhaseScope ph_up(PH_H2D);
    hipError_t e = h->d_row_ptr.upload(row_ptr, n + 1);
    if (e == hipSuccess) e = h->d_col.upload(c.data(), nnz);
    if (e == hipSuccess && !uniform) e = h->d_w.upload(ww.data(), nnz);
    if (e == hipSuccess) e = h->d_start.upload(start.data(), start.size());
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
    h->unigram_ready = false; h->hotkey_state = 0;
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
    h->unigram_ready = false; h->hotkey_state = 0;
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
    h->unigram_ready = false; h->hotkey_state = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_bind_counts(gemhip_n2v_t h, void *d_counts)
{
    GEMHIP_REQUIRE(h && d_counts, "n2v_bind_counts: NULL argument");
    h->counts_own.reset();
    h->d_counts = (int32_t *)d_counts; h->unigram_ready = false; h->hotkey_state = 0;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_pairs(gemhip_n2v_t h, int64_t *pairs, int32_t reset)
{
    GEMHIP_REQUIRE(h && pairs, "sgns_pairs: NULL argument");
    GEMHIP_CHECK(hipDeviceSynchronize());
    unsigned long long v = 0;
    GEMHIP_CHECK(hipMemcpy(&v, h->d_pairs, sizeof v, hipMemcpyDeviceToHost));
    if (reset) GEMHIP_CHECK(hipMemset(h->d_pairs, 0, sizeof v));
    *pairs = (int64_t)v;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_counts_ptr(gemhip_n2v_t h, void **d_counts)
{
    GEMHIP_REQUIRE(h && d_counts, "n2v_counts_ptr: NULL argument");
    *d_counts = h->d_counts;
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ unigram tables
// The four builders below validate, obtain the token counts (and, for the binary's layout, the first-appearance order), call the one host builder
// (sgns_plan.hip build_unigram_tables: Vose per partition, both layouts), upload through the one path of their table set and copy their optional
// outputs in the index space gem_hip.h documents for each.  The handle changes only when a build succeeds.
static int read_counts(gemhip_n2v_t h, std::vector<int32_t> &cnt)
{
    GEMHIP_CHECK(hipDeviceSynchronize());
    cnt.resize(h->n);
    PhaseScope ph(PH_D2H);
    GEMHIP_CHECK(hipMemcpy(cnt.data(), h->d_counts, h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

static int host_tables(const std::vector<int32_t> &cnt, const int32_t *order, int32_t parts, int32_t flags, UnigramTables &T)
{
    PhaseScope ph(PH_HOST);
    return build_unigram_tables(cnt.data(), (int64_t)cnt.size(), order, parts, flags, T);
}

// {bits of U[i], K[i]} interleaved: one 8-byte gather instead of two 4-byte gathers
static std::vector<uint2> interleave_uk(const std::vector<float> &U, const std::vector<int32_t> &K)
{
    std::vector<uint2> UK(U.size());
    for (size_t i = 0; i < U.size(); ++i) { uint32_t ub; memcpy(&ub, &U[i], 4); UK[i] = make_uint2(ub, (uint32_t)K[i]); }
    return UK;
}

// One table set of the handle -- d_UT / d_KT / d_UK / d_KTslot, or the per-partition d_UTp / d_KTp / d_UKp / d_KTslotp: the alias arrays by local row
// (alias_arrays; the single table in the binary's layout is read through UK and the slot table only), their interleave, and the slot table where the
// layout has one (entries beyond a partition's slot count go up as 0; never read: a launch draws slots below that count)
static int upload_unigram(const UnigramTables &T, bool alias_arrays, DevBuf<float> &UT, DevBuf<int32_t> &KT, DevBuf<uint2> &UK, DevBuf<int32_t> &KTslot)
{
    PhaseScope ph(PH_H2D);
    const size_t n = T.U.size();
    const std::vector<uint2> uk = interleave_uk(T.U, T.K);
    std::vector<int32_t> Sdev(T.slot);
    for (auto &v : Sdev) if (v < 0) v = 0;
    if (alias_arrays) { GEMHIP_CHECK(UT.upload(T.U.data(), n)); GEMHIP_CHECK(KT.upload(T.K.data(), n)); }
    GEMHIP_CHECK(UK.upload(uk.data(), n));
    if (!Sdev.empty()) GEMHIP_CHECK(KTslot.upload(Sdev.data(), n));
    return GEMHIP_OK;
}

// ... and what a successful per-partition build leaves on the handle
static void commit_parts(gemhip_n2v_t h, UnigramTables &T, int32_t parts, bool vocab_order)
{
    h->vs = std::move(T.vs); h->vs_part = std::move(T.vs_part); h->part_off = std::move(T.part_off); h->part_slots = std::move(T.part_slots);
    h->parts = parts; h->skp_state = -1; h->parts_vocab_order = vocab_order;
}

extern "C" int gemhip_n2v_build_unigram(gemhip_n2v_t h, int32_t *counts_out, float *UT_out, int32_t *KT_out)
{
    GEMHIP_REQUIRE(h, "n2v_build_unigram: NULL handle");
    std::vector<int32_t> cnt; UnigramTables T;
    if (int rc = read_counts(h, cnt)) return rc;
    GEMHIP_REQUIRE(host_tables(cnt, nullptr, 1, 0, T) < 0, "n2v_build_unigram: empty vocabulary (no walks?)");
    if (int rc = upload_unigram(T, true, h->d_UT, h->d_KT, h->d_UK, h->d_KTslot)) return rc;
    h->vs = std::move(T.vs);
    h->unigram_ready = true; h->vocab_order = false; h->sk_state = -1; h->hotkey_state = 0;
    if (counts_out) std::copy(cnt.begin(), cnt.end(), counts_out);
    if (UT_out) std::copy(T.U.begin(), T.U.end(), UT_out);
    if (KT_out) std::copy(T.K.begin(), T.K.end(), KT_out);
    return GEMHIP_OK;
}

// Nodes in order of first appearance in a token buffer on the device (-1 tokens are padding): back[r] = node with the r-th smallest first token index
// (nodes that never occur sort last), cnt = the handle's token counts.  LearnVocab's renaming (ELF @0x40d560) is r -> back[r] over the nodes that occur.
static int first_appearance_order(gemhip_n2v_t h, const int32_t *d_tokens, int64_t ntok, std::vector<int32_t> &back, std::vector<int32_t> &cnt)
{
    // like its sibling builders: the walks / counts may have been produced on a non-blocking stream of the caller (staged C-ABI use); the launches
    // below go to the null stream, which does not wait for such a stream
    GEMHIP_CHECK(hipDeviceSynchronize());
    const int64_t n = h->n;
    GEMHIP_CHECK(h->d_first.reserve(n));
    GEMHIP_CHECK(hipMemset(h->d_first, 0xff, n * sizeof(unsigned long long)));
    hipLaunchKernelGGL(n2v_first_token_kernel, dim3((unsigned)std::min<int64_t>((ntok + 255) / 256, 256 * 16)), dim3(256), 0, 0, d_tokens, ntok, h->d_first);
    GEMHIP_CHECK(hipGetLastError());
    // nodes sorted by their first token index on the device (radix sort of (first, node) pairs: nodes that never occur sort last)
    back.assign(n, 0); cnt.assign(n, 0);
    DevBuf<unsigned long long> keys_out; DevBuf<int32_t> ids; DevBuf<char> tmp; size_t tmp_bytes = 0;
    hipError_t e = keys_out.reserve(n);
    if (e == hipSuccess) e = ids.reserve(2 * n);
    int32_t *ids_out = ids + n;
    if (e == hipSuccess) { hipLaunchKernelGGL(iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ids, n); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, h->d_first.get(), keys_out.get(), ids.get(), ids_out, (int)n);
    if (e == hipSuccess) e = tmp.reserve(tmp_bytes);
    if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(tmp.get(), tmp_bytes, h->d_first.get(), keys_out.get(), ids.get(), ids_out, (int)n);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) { PhaseScope ph(PH_D2H); e = hipMemcpy(back.data(), ids_out, n * sizeof(int32_t), hipMemcpyDeviceToHost);
                           if (e == hipSuccess) e = hipMemcpy(cnt.data(), h->d_counts, n * sizeof(int32_t), hipMemcpyDeviceToHost); }
    if (e != hipSuccess) return fail(GEMHIP_E_HIP, "first_appearance_order: device sort failed: %s", hipGetErrorString(e));
    return GEMHIP_OK;
}

// InitUnigramTable in the BINARY's layout.  LearnEmbeddings (ELF @0x40ea30) renames the tokens 0..N-1 in order of first appearance in the walk matrix
// (LearnVocab @0x40d560) and builds the alias table over those N entries in that order; RndUnigramInt (@0x40d5f0) then draws a SLOT floor(u N) of that
// table.  Vose's stack discipline makes the table depend on the order of its entries, so the node-id layout of gemhip_n2v_build_unigram is the same
// distribution but not the same table (measured on SBM-1024 with the binary-pinned restatement: -0.33 +- 0.24 % of MAP, profiles/r03_unigram_layout_effect.json).
// Here: first token index per node on the device (atomicMin over the walks), nodes that occur sorted by it (N = their number), Vose over their counts in
// that order, and the result stored in NODE space so that the kernels need no renaming of tokens or tables:
//   KTslot[slot] = node of KTable'[slot]   (flags & 2, the RndUnigramInt quirk; else node of slot)        -- what A.KT points at
//   UK[v]        = {UTable'[r(v)], node of KTable'[r(v)]}   with r(v) the renamed id of node v            -- what A.UK points at
// order_out[N]: node ids in first-appearance order; UT_out / KT_out [N]: the table in RENAMED indices, as the binary holds it (tests compare them
// with oracle/snap_stream.py's).  The walks must be the whole corpus of the handle (single-GPU path).
extern "C" int gemhip_n2v_build_unigram_vocab_order(gemhip_n2v_t h, int32_t flags, int64_t *n_vocab_out, int32_t *order_out, float *UT_out, int32_t *KT_out)
{
    GEMHIP_REQUIRE(h && h->d_walks && h->nwalks > 0, "n2v_build_unigram_vocab_order: no walks");
    std::vector<int32_t> back, cnt; UnigramTables T;             // back: renamed id -> node
    if (int rc = first_appearance_order(h, h->d_walks, h->nwalks * h->walk_len, back, cnt)) return rc;
    GEMHIP_REQUIRE(host_tables(cnt, back.data(), 1, flags, T) < 0, "n2v_build_unigram_vocab_order: empty vocabulary");
    if (int rc = upload_unigram(T, false, h->d_UT, h->d_KT, h->d_UK, h->d_KTslot)) return rc;
    const int64_t N = T.n_vocab;
    h->vs = std::move(T.vs);
    h->n_vocab = N; h->vocab_order = true; h->unigram_ready = true; h->sk_state = -1; h->hotkey_state = 0;
    if (n_vocab_out) *n_vocab_out = N;
    if (order_out) std::copy(back.begin(), back.begin() + N, order_out);
    // the builder stores the table by node; entry r of the binary's table is node back[r], its alias the renamed id of that node's alias
    if (UT_out) for (int64_t r = 0; r < N; ++r) UT_out[r] = T.U[back[r]];
    if (KT_out) {
        std::vector<int32_t> renamed(h->n, 0);
        for (int64_t r = 0; r < N; ++r) renamed[back[r]] = (int32_t)r;
        for (int64_t r = 0; r < N; ++r) KT_out[r] = renamed[T.K[back[r]]];
    }
    return GEMHIP_OK;
}

// One alias table per partition p = {v : v % parts == p} over local indices v / parts (restricted unigram).
extern "C" int gemhip_n2v_build_unigram_parts(gemhip_n2v_t h, int32_t parts, float *UT_out, int32_t *KT_out)
{
    GEMHIP_REQUIRE(h && parts >= 1 && parts <= h->n, "n2v_build_unigram_parts: bad arguments");
    std::vector<int32_t> cnt; UnigramTables T;
    if (int rc = read_counts(h, cnt)) return rc;
    const int empty = host_tables(cnt, nullptr, parts, 0, T);
    GEMHIP_REQUIRE(empty < 0, "n2v_build_unigram_parts: partition %d has an empty vocabulary", empty);
    if (int rc = upload_unigram(T, true, h->d_UTp, h->d_KTp, h->d_UKp, h->d_KTslotp)) return rc;
    if (UT_out) std::copy(T.U.begin(), T.U.end(), UT_out);
    if (KT_out) std::copy(T.K.begin(), T.K.end(), KT_out);
    commit_parts(h, T, parts, false);
    return GEMHIP_OK;
}

// The per-partition tables in the BINARY's layout (flags bit GEMHIP_N2V_VOCAB_ORDER on the N-GPU schedule): partition p = the nodes v % parts == p that
// occur, in order of first appearance in the whole corpus -- d_corpus: the walks of ALL ranks in walk-id order (rank-major shards, -1 tokens = padding;
// NULL = this handle's own walks: one rank) -- Vose over their counts (the handle's counts: summed over the ranks) in that order; the slot table and the
// alias arrays are stored by LOCAL row v / parts like the node-id layout's.  With one partition this IS gemhip_n2v_build_unigram_vocab_order's table (the same call of the host builder).
// Optional outputs: UT_out / KT_out [n] by local row (concatenated partitions, as d_UTp / d_KTp), slot_out [n] (partition p's slots at part_off[p],
// -1 beyond its slot count), nslots_out [parts].
extern "C" int gemhip_n2v_build_unigram_parts_vocab_order(gemhip_n2v_t h, int32_t parts, int32_t flags, const void *d_corpus, int64_t corpus_tokens,
                                                          float *UT_out, int32_t *KT_out, int32_t *slot_out, int64_t *nslots_out)
{
    GEMHIP_REQUIRE(h && parts >= 1 && parts <= h->n, "n2v_build_unigram_parts_vocab_order: bad arguments");
    GEMHIP_REQUIRE(d_corpus ? corpus_tokens > 0 : (h->d_walks && h->nwalks > 0), "n2v_build_unigram_parts_vocab_order: no walks");
    std::vector<int32_t> back, cnt; UnigramTables T;
    if (int rc = first_appearance_order(h, d_corpus ? (const int32_t *)d_corpus : h->d_walks, d_corpus ? corpus_tokens : h->nwalks * h->walk_len, back, cnt)) return rc;
    const int empty = host_tables(cnt, back.data(), parts, flags, T);
    GEMHIP_REQUIRE(T.n_vocab > 0, "n2v_build_unigram_parts_vocab_order: empty vocabulary");
    GEMHIP_REQUIRE(empty < 0, "n2v_build_unigram_parts_vocab_order: partition %d has an empty vocabulary", empty);
    if (int rc = upload_unigram(T, true, h->d_UTp, h->d_KTp, h->d_UKp, h->d_KTslotp)) return rc;
    if (UT_out) std::copy(T.U.begin(), T.U.end(), UT_out);
    if (KT_out) std::copy(T.K.begin(), T.K.end(), KT_out);
    if (slot_out) std::copy(T.slot.begin(), T.slot.end(), slot_out);
    if (nslots_out) std::copy(T.part_slots.begin(), T.part_slots.end(), nslots_out);
    commit_parts(h, T, parts, true);
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_init(gemhip_n2v_t h, int32_t d, uint64_t seed, void *dSynPos, void *dSynNeg)
{
    GEMHIP_REQUIRE(h && d >= 1, "sgns_init: bad arguments");
    GEMHIP_REQUIRE(pick_sgns(d) != nullptr, "sgns_init: d=%d unsupported (even d <= 512, odd d <= 256)", d);
    GEMHIP_REQUIRE((dSynPos == nullptr) == (dSynNeg == nullptr), "sgns_init: pass both or neither external table");
    h->syn_own[0].reset(); h->syn_own[1].reset(); h->SynPos = h->SynNeg = nullptr;
    if (!dSynPos) for (auto &b : h->syn_own) GEMHIP_CHECK(b.reserve((size_t)h->n * d));
    h->SynPos = dSynPos ? (float *)dSynPos : h->syn_own[0].get(); h->SynNeg = dSynPos ? (float *)dSynNeg : h->syn_own[1].get();
    h->d = d;
    const int64_t total = h->n * (int64_t)d;
    const int64_t threads = (total + 3) / 4;
    hipLaunchKernelGGL(sgns_init_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, 0, h->SynPos, h->SynNeg, total, d, seed);
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_tables(gemhip_n2v_t h, const float *SynPos_host, const float *SynNeg_host)
{
    GEMHIP_REQUIRE(h && h->SynPos && SynPos_host && SynNeg_host, "sgns_set_tables: bad arguments (call sgns_init first)");
    const size_t bytes = (size_t)h->n * h->d * sizeof(float);
    GEMHIP_CHECK(hipMemcpy(h->SynPos, SynPos_host, bytes, hipMemcpyHostToDevice));
    GEMHIP_CHECK(hipMemcpy(h->SynNeg, SynNeg_host, bytes, hipMemcpyHostToDevice));
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_get_tables(gemhip_n2v_t h, float *SynPos_host, float *SynNeg_host)
{
    GEMHIP_REQUIRE(h && h->SynPos, "sgns_get_tables: no tables");
    GEMHIP_CHECK(hipDeviceSynchronize());
    const size_t bytes = (size_t)h->n * h->d * sizeof(float);
    PhaseScope ph(PH_D2H);
    if (SynPos_host) GEMHIP_CHECK(hipMemcpy(SynPos_host, h->SynPos, bytes, hipMemcpyDeviceToHost));
    if (SynNeg_host) GEMHIP_CHECK(hipMemcpy(SynNeg_host, h->SynNeg, bytes, hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

// LOCALLY HOT ROWS: the array the Hogwild kernels compare with hot_thr -- the token count, or INT32_MAX for a node whose tokens are packed into few walks
// (kernels above).  Built on `stream` from `rows` walks of walk_len tokens (rows of -1 tokens count nothing) and the handle's (possibly externally
// reduced) counts; n_local_hot is read back (one 4-byte copy): a launch without any such node and without count-hot rows keeps the all-cached
// instantiation.  state: what hotkey_state becomes -- 1 built from the handle's own walks, 2 from a gathered corpus.
static int build_hotkey(gemhip_n2v_t h, const int32_t *walks, int64_t rows, int32_t walk_len, hipStream_t stream, int state)
{
    GEMHIP_CHECK(h->d_hotkey.reserve(h->n));
    GEMHIP_CHECK(h->d_wcount.reserve(h->n));
    GEMHIP_CHECK(h->d_nlocal.reserve(1));
    GEMHIP_CHECK(hipMemsetAsync(h->d_wcount, 0, (size_t)h->n * sizeof(int32_t), stream));
    GEMHIP_CHECK(hipMemsetAsync(h->d_nlocal, 0, sizeof(unsigned int), stream));
    if (rows > 0) {
        const int64_t blocks = std::min<int64_t>(rows, 256 * 32);
        hipLaunchKernelGGL(n2v_walk_presence_kernel, dim3((unsigned)blocks), dim3(64), (size_t)walk_len * sizeof(int32_t), stream, walks, rows, walk_len, h->d_wcount);
    }
    hipLaunchKernelGGL(n2v_hotkey_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, stream, h->n, h->d_counts, h->d_wcount, h->kn.local_hot, h->d_hotkey, h->d_nlocal);
    GEMHIP_CHECK(hipGetLastError());
    unsigned int nl = 0;
    GEMHIP_CHECK(hipMemcpyAsync(&nl, h->d_nlocal, sizeof nl, hipMemcpyDeviceToHost, stream));
    GEMHIP_CHECK(hipStreamSynchronize(stream));
    h->n_local_hot = nl;
    h->hotkey_state = state;
    return GEMHIP_OK;
}
// ... of the walks this handle holds: rebuilt after walks / vocabulary change
static int ensure_hotkey(gemhip_n2v_t h, hipStream_t stream)
{
    return h->hotkey_state == 1 ? GEMHIP_OK : build_hotkey(h, h->d_walks, h->nwalks, h->walk_len, stream, 1);
}

// The slot table the window kernels draw negatives from (SgnsArgs::SK), for the table currently held and the given quirk bit.  Built on `stream`,
// in front of the launch that needs it; rebuilt only after a table build or when the quirk bit changes.
static int ensure_slot_table(gemhip_n2v_t h, const int32_t *KT, int64_t nslots, int quirk, hipStream_t stream)
{
    if (h->sk_state == quirk && h->d_SK) return GEMHIP_OK;
    GEMHIP_CHECK(h->d_SK.reserve(nslots));
    hipLaunchKernelGGL(n2v_slot_table_kernel, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, stream, nslots, KT, h->d_UK, quirk, h->d_SK);
    GEMHIP_CHECK(hipGetLastError());
    h->sk_state = quirk;
    return GEMHIP_OK;
}
// ... and of the per-partition tables: partition p's slots occupy [part_off[p], part_off[p+1]) of d_SKp, entries in LOCAL indices like d_KTp / d_UKp
static int ensure_slot_table_parts(gemhip_n2v_t h, int quirk, hipStream_t stream)
{
    if (h->skp_state == quirk && h->d_SKp) return GEMHIP_OK;
    GEMHIP_CHECK(h->d_SKp.reserve(h->n));
    for (int32_t p = 0; p < h->parts; ++p) {
        const int64_t off = h->part_off[p], np = h->parts_vocab_order ? h->part_slots[p] : h->part_off[p + 1] - off;
        if (np <= 0) continue;
        // (the binary's layout: the slot table names the entry -- quirk already folded in --, the alias arrays are indexed by local row)
        hipLaunchKernelGGL(n2v_slot_table_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, np, (h->parts_vocab_order ? h->d_KTslotp : h->d_KTp) + off,
                           h->d_UKp + off, h->parts_vocab_order ? 1 : quirk, h->d_SKp + off);
    }
    GEMHIP_CHECK(hipGetLastError());
    h->skp_state = quirk;
    return GEMHIP_OK;
}

// The per-wavefront rows of the window kernels: one scratch row each (SgnsArgs::dummy, zeroed when it is allocated) and, for the delta write-back
// of sgns_win_kernel<PART>, the 2R+1 window rows as loaded (SgnsArgs::scratch).  Grow-only: a launch that fits what is held makes no HIP call.
static int ensure_win_scratch(gemhip_n2v_t h, const SgnsLaunchPlan &P, int32_t d, bool part_delta, SgnsArgs &A)
{
    const size_t need = (size_t)P.waves * sgns_win_row_floats(d);
    if (need > h->d_dummy.capacity()) {
        GEMHIP_CHECK(h->d_dummy.reserve(need));
        GEMHIP_CHECK(hipMemset(h->d_dummy, 0, need * sizeof(float)));
    }
    A.dummy = h->d_dummy;
    if (part_delta) GEMHIP_CHECK(h->d_scratch.reserve(need * (size_t)(2 * P.R + 1)));
    A.scratch = part_delta ? h->d_scratch.get() : nullptr;
    return GEMHIP_OK;
}

// Instrumentation builds (scripts/build_variant.sh with -DGEMHIP_SGNS_STALENESS / -DGEMHIP_SGNS_PROFILE): device counters a window launch of
// gemhip_sgns_train carries (begin) and the line printed once it has run (report).  The product build compiles neither.
#ifdef GEMHIP_SGNS_STALENESS
static int staleness_begin(gemhip_n2v_t h, SgnsArgs &A)
{
    static unsigned int *d_sver = nullptr; static unsigned long long *d_shist = nullptr; static int64_t sver_n = 0;
    if (sver_n < h->n) { if (d_sver) hipFree(d_sver); GEMHIP_CHECK(hipMalloc(&d_sver, (size_t)h->n * 2 * sizeof(unsigned int))); sver_n = h->n; }
    if (!d_shist) GEMHIP_CHECK(hipMalloc(&d_shist, 3 * 32 * 16 * sizeof(unsigned long long)));
    GEMHIP_CHECK(hipMemset(d_sver, 0, (size_t)h->n * 2 * sizeof(unsigned int)));
    GEMHIP_CHECK(hipMemset(d_shist, 0, 3 * 32 * 16 * sizeof(unsigned long long)));
    A.stale_ver = d_sver; A.stale_hist = d_shist;
    return GEMHIP_OK;
}
// one JSON line per launch: {"waves", "hot_thr", "fresh", "hist": {class: {log2 count: [launches by bit length of the foreign-update count]}}}
static int staleness_report(gemhip_n2v_t h, const SgnsLaunchPlan &P, const SgnsArgs &A)
{
    std::vector<unsigned long long> hh(3 * 32 * 16);
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(hipMemcpy(hh.data(), A.stale_hist, hh.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    FILE *fo = getenv("GEMHIP_SGNS_STALENESS_OUT") ? fopen(getenv("GEMHIP_SGNS_STALENESS_OUT"), "a") : stderr;
    if (fo) {
        fprintf(fo, "{\"waves\": %lld, \"hot_thr\": %d, \"fresh\": %d, \"vocab_order\": %d, \"hist\": {", (long long)P.waves, (int)P.hot_thr, (int)A.fresh, (int)h->vocab_order);
        const char *cls[3] = {"negative", "centre", "context"};
        for (int c = 0; c < 3; ++c) {
            fprintf(fo, "%s\"%s\": {", c ? ", " : "", cls[c]);
            bool first = true;
            for (int hb = 0; hb < 32; ++hb) {
                unsigned long long tot = 0; for (int sb = 0; sb < 16; ++sb) tot += hh[(c * 32 + hb) * 16 + sb];
                if (!tot) continue;
                fprintf(fo, "%s\"%d\": [", first ? "" : ", ", hb); first = false;
                for (int sb = 0; sb < 16; ++sb) fprintf(fo, "%s%llu", sb ? ", " : "", hh[(c * 32 + hb) * 16 + sb]);
                fprintf(fo, "]");
            }
            fprintf(fo, "}");
        }
        fprintf(fo, "}}\n");
        if (fo != stderr) fclose(fo);
    }
    return GEMHIP_OK;
}
#else
static int staleness_begin(gemhip_n2v_t, SgnsArgs &) { return GEMHIP_OK; }
static int staleness_report(gemhip_n2v_t, const SgnsLaunchPlan &, const SgnsArgs &) { return GEMHIP_OK; }
#endif
#ifdef GEMHIP_SGNS_PROFILE
static int profile_begin(SgnsArgs &A)
{
    static unsigned long long *d_prof = nullptr;
    if (!d_prof) GEMHIP_CHECK(hipMalloc(&d_prof, 64));
    GEMHIP_CHECK(hipMemset(d_prof, 0, 64));
    A.prof = d_prof;
    return GEMHIP_OK;
}
static int profile_report(const SgnsLaunchPlan &P, const SgnsArgs &A)
{
    unsigned long long hp[8];
    GEMHIP_CHECK(hipDeviceSynchronize());
    GEMHIP_CHECK(hipMemcpy(hp, A.prof, 64, hipMemcpyDeviceToHost));
    fprintf(stderr, "[sgns profile] waves=%lld cycles: other=%llu issue=%llu ctx_lds=%llu wait_rows=%llu compute_store=%llu neg_pipeline=%llu centre_setup=%llu centre_end=%llu\n",
            (long long)P.waves, hp[0], hp[1], hp[2], hp[3], hp[4], hp[5], hp[6], hp[7]);
    return GEMHIP_OK;
}
#else
static int profile_begin(SgnsArgs &) { return GEMHIP_OK; }
static int profile_report(const SgnsLaunchPlan &, const SgnsArgs &) { return GEMHIP_OK; }
#endif

// What gemhip_sgns_train and gemhip_sgns_train_part hand the kernels alike (every other field keeps SgnsArgs' default until its entry point sets it): the
// walks and the range of work items, alpha's schedule, the Philox keys, the embedding tables, the handle's pair counter and fresh-row knobs, and the
// unigram table the negatives are drawn from -- the handle's single table (word_part < 0) or the one of partition word_part, in the layout it was built in
static SgnsArgs sgns_args(gemhip_n2v_t h, int32_t word_part, const int32_t *walks, int64_t walk_lo, int64_t walk_hi, int32_t walk_len, int32_t window, float alpha0,
                          int64_t denom, int64_t token_offset, int64_t walk_id_offset, int32_t epoch, uint64_t seed, int32_t flags, int32_t d, float *SynPos, float *SynNeg)
{
    SgnsArgs A;
    A.walks = walks; A.walk_lo = walk_lo; A.walk_hi = walk_hi; A.walk_len = walk_len; A.window = window;
    // the kernel computes t = token_offset + wl*walk_len + pos with wl the index of the work item
    A.alpha0 = alpha0; A.denom = denom; A.token_offset = token_offset; A.walk_id_offset = walk_id_offset; A.epoch = epoch;
    A.seed = seed; A.flags = flags; A.d = d;
    const bool part = word_part >= 0;
    const int64_t off = part ? h->part_off[word_part] : 0;
    A.UT = (part ? h->d_UTp : h->d_UT) + off; A.KT = (part ? h->d_KTp : h->d_KT) + off; A.UK = (part ? h->d_UKp : h->d_UK) + off;
    A.n = (uint32_t)(part ? h->part_off[word_part + 1] - off : h->n);
    if (part ? h->parts_vocab_order : h->vocab_order) {      // the binary's table layout: slots over the (partition's) nodes that occur, in first-appearance order; the slot table is always consulted
        A.KT = (part ? h->d_KTslotp : h->d_KTslot) + off; A.n = (uint32_t)(part ? h->part_slots[word_part] : h->n_vocab); A.flags = flags | 2; A.UT = nullptr;
    }
    A.SynPos = SynPos; A.SynNeg = SynNeg; A.pairs = h->d_pairs;
    A.fresh = h->kn.fresh; A.neg_thr = h->kn.neg_count; A.n_nodes = h->n;
    return A;
}

extern "C" int gemhip_sgns_train(gemhip_n2v_t h, int32_t window, int32_t neg, float alpha0, int32_t epochs, int32_t epoch,
                                 int64_t walk_lo, int64_t walk_hi, int64_t tokens_total, int64_t token_offset, uint64_t seed,
                                 int32_t flags, void *stream)
{
    GEMHIP_REQUIRE(h && h->SynPos, "sgns_train: call sgns_init first");
    GEMHIP_REQUIRE(h->unigram_ready, "sgns_train: call n2v_vocab + n2v_build_unigram first");
    GEMHIP_REQUIRE(neg == SGNS_NEG, "sgns_train: neg=%d unsupported (the reference binary fixes NegSamN=5)", neg);
    GEMHIP_REQUIRE(window >= 1 && window < 16384, "sgns_train: window=%d", window);
    GEMHIP_REQUIRE(epochs >= 1 && epoch >= 0 && epoch < epochs && epoch < 256, "sgns_train: epoch %d of %d", epoch, epochs);
    GEMHIP_REQUIRE(0 <= walk_lo && walk_lo <= walk_hi && walk_hi <= h->nwalks, "sgns_train: bad local walk range");
    GEMHIP_REQUIRE(tokens_total >= 1, "sgns_train: tokens_total=%lld", (long long)tokens_total);
    if (walk_hi == walk_lo) return GEMHIP_OK;
    SgnsArgs A = sgns_args(h, -1, h->d_walks, walk_lo, walk_hi, h->walk_len, window, alpha0, (int64_t)epochs * tokens_total + 1, token_offset, h->walk_id_offset,
                           epoch, seed, flags, h->d, h->SynPos, h->SynNeg);
    A.prefetch = h->kn.prefetch; A.reload = h->kn.reload;
    SgnsKnobs kn_launch = h->kn;
    kn_launch.node_id_layout = !h->vocab_order;
    // LOCALLY HOT ROWS need the WHOLE corpus on this handle (walks-per-node is a property of the corpus: a rank's shard against all-reduced counts would
    // flag everything); Hogwild launches only
    if (!(flags & 4) && h->kn.local_hot > 0 && h->walk_id_offset == 0 && h->vs.total <= (double)h->nwalks * h->walk_len + 0.5) {
        { const int rc = ensure_hotkey(h, (hipStream_t)stream); if (rc) return rc; }
        kn_launch.has_local_hot = h->n_local_hot > 0;
    }
    const SgnsLaunchPlan P = plan_sgns_launch(h->vs, kn_launch, h->n, h->d, window, h->walk_len, walk_hi - walk_lo, flags);
    GEMHIP_REQUIRE(P.lds <= 64 * 1024, "sgns_train: walk_len/window/d too large for LDS staging (%zu bytes)", P.lds);
    A.nwaves = (int32_t)P.waves; A.cache_radius = P.R;
    if (P.window) {
        { const int rc = ensure_slot_table(h, A.KT, (int64_t)A.n, (A.flags & 2) ? 1 : 0, (hipStream_t)stream); if (rc) return rc; }
        A.SK = h->d_SK;
        // hot rows (sgns_win_kernel): never cached; the launch then takes the instantiation that handles uncached contexts
        A.counts = h->d_counts; A.hot_thr = P.hot_thr;
        // LOCALLY HOT ROWS: the kernel compares `hotkey` (INT32_MAX for a node whose tokens are packed into few walks, else its token count) with the threshold
        if (P.delta && P.waves > 1 && kn_launch.has_local_hot) A.counts = h->d_hotkey;
        { const int rc = ensure_win_scratch(h, P, h->d, false, A); if (rc) return rc; }
        if (int rc = staleness_begin(h, A)) return rc;
        if (int rc = profile_begin(A)) return rc;
    }
    sgns_fn fn = !P.window ? pick_sgns(h->d) : P.delta ? pick_sgns_win_hogwild(h->d) : pick_sgns_win_det(h->d);
    GEMHIP_REQUIRE(fn != nullptr, "sgns_train: d=%d unsupported", h->d);
    h->last_plan = P; h->last_fresh = (P.window && P.delta && P.hot_thr > 0) ? A.fresh : 0;
    fn(A, P.blocks, P.threads, P.lds, (hipStream_t)stream);
    GEMHIP_CHECK(hipGetLastError());
    if (P.window) {
        if (int rc = staleness_report(h, P, A)) return rc;
        if (int rc = profile_report(P, A)) return rc;
    }
    return GEMHIP_OK;
}

// The launch plan for the given token counts, without a device: what gemhip_sgns_train would do on a handle with default knobs (tests/test_sgns_plan.py).
extern "C" int gemhip_sgns_plan_launch(const int32_t *counts, int64_t n, int32_t d, int32_t window, int32_t walk_len, int64_t nwalks, int32_t flags,
                                       int32_t *kernel, int32_t *waves, int32_t *hot_threshold, double *n_eff, double *n_eff_cold)
{
    GEMHIP_REQUIRE(counts && n >= 1 && d >= 1 && window >= 1 && walk_len >= 1 && nwalks >= 1, "sgns_plan_launch: bad arguments");
    VocabStats vs;
    vs.build(counts, n);
    SgnsKnobs kn;
    kn.node_id_layout = !(flags & GEMHIP_N2V_VOCAB_ORDER);
    const SgnsLaunchPlan P = plan_sgns_launch(vs, kn, n, d, window, walk_len, nwalks, flags);
    if (kernel) *kernel = P.kernel();
    if (waves) *waves = (int32_t)P.waves;
    if (hot_threshold) *hot_threshold = P.hot_thr;
    if (n_eff) *n_eff = vs.n_eff;
    if (n_eff_cold) *n_eff_cold = P.hot_thr > 0 ? vs.n_eff_cold((double)P.hot_thr) : vs.n_eff;
    return GEMHIP_OK;
}

// One bucket of the partitioned (N-GPU) schedule trained in WALK order: TrainModel over a walk corpus restricted to the pairs whose context lies in
// partition ctx_part (rows of dSynPos_part) and whose centre word lies in partition word_part (rows of dSynNeg_part; negatives drawn from the unigram
// table restricted to word_part).  The corpus may be assembled from several ranks' shards (d_seg: nseg segments, see SgnsArgs::seg); alpha follows
// the index of the token in the work-item order (token_offset + index).  Same kernel, same draws per (walk id, position) as gemhip_sgns_train: with
// parts == 1 it IS gemhip_sgns_train.  Replaces the pair-list pipeline (emit -> bucket -> all-to-all -> sgns_pairs_kernel) of rounds 2-3: what a
// rank needs from the others is their walks (4 bytes per token, once), not pairs (80 bytes per token, every episode), and the order of the pairs
// inside a bucket is the reference's.
extern "C" int gemhip_sgns_train_part(gemhip_n2v_t h, const void *d_walks, int64_t nwalks, int32_t walk_len, const void *d_seg, int32_t nseg,
                                      int64_t seg_len, int64_t walk_id_offset, int32_t window, float alpha0, int64_t alpha_tokens_total,
                                      int64_t token_offset, int32_t epoch, uint64_t seed, int32_t flags, int32_t ctx_part, int32_t word_part,
                                      void *dSynPos_part, void *dSynNeg_part, int32_t d, void *stream)
{
    GEMHIP_REQUIRE(h && h->parts >= 1, "sgns_train_part: call n2v_build_unigram_parts first");
    GEMHIP_REQUIRE(nwalks >= 0 && (nwalks == 0 || d_walks) && walk_len >= 1 && walk_len < 65536 && dSynPos_part && dSynNeg_part, "sgns_train_part: bad arguments");
    GEMHIP_REQUIRE(ctx_part >= 0 && ctx_part < h->parts && word_part >= 0 && word_part < h->parts, "sgns_train_part: partitions (%d, %d) of %d", ctx_part, word_part, h->parts);
    GEMHIP_REQUIRE(window >= 1 && window < 16384 && epoch >= 0 && epoch < 256 && alpha_tokens_total >= 1, "sgns_train_part: window=%d epoch=%d", window, epoch);
    GEMHIP_REQUIRE(d_seg == nullptr || (nseg >= 1 && seg_len >= 1 && nwalks == (int64_t)nseg * seg_len), "sgns_train_part: nseg=%d seg_len=%lld nwalks=%lld (need nwalks == nseg * seg_len work items)",
                   nseg, (long long)seg_len, (long long)nwalks);
    GEMHIP_REQUIRE((h->n + h->parts - 1) / h->parts < (int64_t)(1 << 29), "sgns_train_part: more than 2^29 rows per partition");
    if (nwalks == 0) return GEMHIP_OK;
    SgnsArgs A = sgns_args(h, word_part, (const int32_t *)d_walks, 0, nwalks, walk_len, window, alpha0, alpha_tokens_total + 1, token_offset, walk_id_offset, epoch, seed,
                           flags, d, (float *)dSynPos_part, (float *)dSynNeg_part);
    if (int rc = ensure_slot_table_parts(h, (A.flags & 2) ? 1 : 0, (hipStream_t)stream)) return rc;
    A.SK = h->d_SKp + h->part_off[word_part];
    A.counts = h->d_counts;
    A.parts = h->parts; A.ctx_part = ctx_part; A.word_part = word_part; A.seg = (const int64_t *)d_seg; A.nseg = nseg; A.seg_len = seg_len;
    VocabStats vs;
    const SgnsKnobs kn = bucket_knobs(h->kn, h->vs_part[word_part], h->vs, h->parts, walk_len, window, flags, !h->parts_vocab_order, h->hotkey_state == 2 && h->n_local_hot > 0, &vs);
    const SgnsLaunchPlan P = plan_sgns_launch(vs, kn, (int64_t)A.n, d, window, walk_len, nwalks, flags);
    GEMHIP_REQUIRE(P.window, "sgns_train_part: d=%d window=%d walk_len=%d do not fit the LDS window kernel", d, window, walk_len);
    A.nwaves = (int32_t)P.waves; A.cache_radius = P.R; A.hot_thr = P.hot_thr;
    if (kn.has_local_hot && P.delta && P.waves > 1) A.counts = h->d_hotkey;
    { const int rc = ensure_win_scratch(h, P, d, P.delta, A); if (rc) return rc; }
    sgns_fn fn = pick_sgns_win_part(d, P.delta);
    GEMHIP_REQUIRE(fn != nullptr, "sgns_train_part: d=%d unsupported", d);
    h->last_plan = P; h->last_fresh = (P.delta && P.hot_thr > 0) ? A.fresh : 0;
    fn(A, P.blocks, P.threads, P.lds, (hipStream_t)stream);
    GEMHIP_CHECK(hipGetLastError());
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

namespace {
__global__ void wave_sum6_test_kernel(const float *in, float *out)
{
    const int lane = lane_id();
    float p[6];
    for (int k = 0; k < 6; ++k) p[k] = in[lane * 6 + k];
    out[lane] = wave_sum6(p, lane);
}
}  // namespace

// Building block exposed for its own parity test: in[64][6] partial sums of one wavefront -> out[64], lane l receiving the
// wave total of value (l & 4) ? 4 + (l & 1) : (l & 3).
extern "C" int gemhip_test_wave_sum6(const float *in_host, float *out_host)
{
    GEMHIP_REQUIRE(in_host && out_host, "test_wave_sum6: NULL argument");
    DevBuf<float> d;
    GEMHIP_CHECK(d.reserve(64 * 6 + 64));
    hipError_t e = hipMemcpy(d, in_host, 64 * 6 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) { hipLaunchKernelGGL(wave_sum6_test_kernel, dim3(1), dim3(64), 0, 0, d, d + 64 * 6); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpy(out_host, d + 64 * 6, 64 * sizeof(float), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(GEMHIP_E_HIP, "test_wave_sum6: %s", hipGetErrorString(e));
    return GEMHIP_OK;
}

// ... the same key from a walk CORPUS assembled from every rank's shard (the partitioned N-GPU schedule: gemhip_sgns_train_part trains buckets of it), with
// the handle's -- all-reduced -- token counts: rows of -1 tokens (padding of shorter shards) count nothing.  Bucket launches on this handle then treat the
// locally hot nodes as hot rows (hotkey is indexed by GLOBAL node id, like the counts the bucket kernels read).
extern "C" int gemhip_n2v_locally_hot_corpus(gemhip_n2v_t h, const void *d_corpus, int64_t corpus_rows, int32_t walk_len, int32_t per_walk, int64_t *count, void *stream)
{
    GEMHIP_REQUIRE(h && d_corpus && corpus_rows >= 1 && walk_len >= 1 && per_walk >= -1, "n2v_locally_hot_corpus: bad arguments");
    if (per_walk >= 0) h->kn.local_hot = per_walk;
    h->hotkey_state = 0; h->n_local_hot = 0;
    if (h->kn.local_hot == 0) { if (count) *count = 0; return GEMHIP_OK; }
    // (state 2: gemhip_sgns_train_part uses it; gemhip_sgns_train rebuilds its own from the handle's walks)
    if (int rc = build_hotkey(h, (const int32_t *)d_corpus, corpus_rows, walk_len, (hipStream_t)stream, 2)) return rc;
    if (count) *count = h->n_local_hot;
    return GEMHIP_OK;
}

extern "C" int gemhip_n2v_locally_hot(gemhip_n2v_t h, int32_t per_walk, int64_t *count, int32_t *hotkey_host)
{
    GEMHIP_REQUIRE(h && per_walk >= -1, "n2v_locally_hot: bad arguments");
    GEMHIP_REQUIRE(h->d_walks && h->nwalks > 0, "n2v_locally_hot: no walks on this handle");
    if (per_walk >= 0 && per_walk != h->kn.local_hot) { h->kn.local_hot = per_walk; h->hotkey_state = 0; }
    if (h->kn.local_hot == 0) {            // off: nothing is locally hot, the key is the token count
        if (count) *count = 0;
        if (hotkey_host) GEMHIP_CHECK(hipMemcpy(hotkey_host, h->d_counts, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
        return GEMHIP_OK;
    }
    { const int rc = ensure_hotkey(h, nullptr); if (rc) return rc; }
    if (count) *count = h->n_local_hot;
    if (hotkey_host) GEMHIP_CHECK(hipMemcpy(hotkey_host, h->d_hotkey, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_last_launch(gemhip_n2v_t h, int32_t *kernel, int32_t *waves, int32_t *hot_threshold, int32_t *fresh)
{
    GEMHIP_REQUIRE(h, "sgns_last_launch: null handle");
    const SgnsLaunchPlan &P = h->last_plan;
    if (kernel) *kernel = P.kernel();
    if (waves) *waves = (int32_t)P.waves;
    if (hot_threshold) *hot_threshold = P.hot_thr;
    if (fresh) *fresh = h->last_fresh;
    return GEMHIP_OK;
}

// ------------------------------------------------------------------ launch knobs (per handle; the environment overrides are read once, in gemhip_n2v_create)
extern "C" int gemhip_n2v_set_max_waves(gemhip_n2v_t h, int32_t max_waves)
{
    GEMHIP_REQUIRE(h && max_waves >= 0, "n2v_set_max_waves: bad arguments");
    h->kn.max_waves = max_waves;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_window_cache(gemhip_n2v_t h, int32_t radius, int32_t delta_writeback)
{
    GEMHIP_REQUIRE(h && radius >= -1 && radius <= 31 && delta_writeback >= -1 && delta_writeback <= 1, "sgns_set_window_cache: bad arguments");
    h->kn.cache_radius = radius;
    h->kn.cache_delta = delta_writeback;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_hogwild(gemhip_n2v_t h, int32_t prefetch_pairs, int32_t reload_on_update)
{
    GEMHIP_REQUIRE(h && prefetch_pairs >= 0 && prefetch_pairs <= 2 && reload_on_update >= -1 && reload_on_update <= 1, "sgns_set_hogwild: bad arguments");
    if (prefetch_pairs) h->kn.prefetch = prefetch_pairs;
    if (reload_on_update >= 0) h->kn.reload = reload_on_update;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_hot_rows(gemhip_n2v_t h, int32_t min_count)
{
    GEMHIP_REQUIRE(h && min_count >= -1, "sgns_set_hot_rows: bad arguments");
    h->kn.hot_count = min_count;
    return GEMHIP_OK;
}

extern "C" int gemhip_sgns_set_fresh(gemhip_n2v_t h, int32_t bits)
{
    GEMHIP_REQUIRE(h && bits >= 0 && bits <= 7, "sgns_set_fresh: bits=%d (0..7)", bits);
    h->kn.fresh = bits;
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
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (auto &e : ev) if (!rc && hipEventCreate(&e) != hipSuccess) rc = fail(GEMHIP_E_HIP, "n2v_train: hipEventCreate");
    const int64_t nwalks = h->m_start * (int64_t)num_walks;
    if (!rc) { hipEventRecord(ev[0], 0); rc = gemhip_n2v_walks(h, p, q, num_walks, walk_len, seed, flags, 0, nwalks, nullptr); }
    if (!rc) rc = gemhip_n2v_vocab(h, nullptr);
    if (!rc) { hipEventRecord(ev[1], 0); rc = (flags & GEMHIP_N2V_VOCAB_ORDER) ? gemhip_n2v_build_unigram_vocab_order(h, flags, nullptr, nullptr, nullptr, nullptr)
                                                                                 : gemhip_n2v_build_unigram(h, nullptr, nullptr, nullptr); }
    if (!rc) rc = gemhip_sgns_init(h, d, seed, nullptr, nullptr);
    if (!rc) hipEventRecord(ev[2], 0);
    for (int ep = 0; !rc && ep < epochs; ++ep)
        rc = gemhip_sgns_train(h, window, SGNS_NEG, 0.025f, epochs, ep, 0, nwalks, nwalks * walk_len, (int64_t)ep * nwalks * walk_len,
                               seed, flags, nullptr);
    if (!rc) { hipEventRecord(ev[3], 0); rc = gemhip_sgns_get_tables(h, X_out, nullptr); }
    if (!rc && stats) {
        float a = 0, b = 0;
        hipEventElapsedTime(&a, ev[0], ev[1]);
        hipEventElapsedTime(&b, ev[2], ev[3]);
        stats[0] = a * 1e-3; stats[1] = b * 1e-3; stats[2] = (double)nwalks * walk_len; stats[3] = h->uniform_rows ? 1.0 : 0.0;
    }
    if (!rc) {     // kernel seconds of the call (HIP events): walks + vocabulary, then table init + SGNS
        float a = 0, b = 0;
        hipEventElapsedTime(&a, ev[0], ev[1]);
        hipEventElapsedTime(&b, ev[2], ev[3]);
        phase_acc()[PH_KERNELS] = (a + b) * 1e-3;
    }
    for (auto &e : ev) if (e) hipEventDestroy(e);
    gemhip_n2v_destroy(h);
    phase_acc()[PH_TOTAL] = phase_now() - t_call;
    return rc;
}
