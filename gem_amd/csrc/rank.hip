// rank.hip -- a device sort of fp64 scores and the exact binary ranking metrics on top of it: ROC-AUC, average
// precision, the ROC / PR curve points.  The host arithmetic (keys, checks, which passes to skip, the metrics from a group table) is
// rank_host.hip.
//
// Sort.  A stable least-significant-digit radix sort of the 64-bit keys (rank_host.hpp: ascending key = descending score, -0.0 = +0.0) with
// the int32 position as payload, RANK_PASSES = 8 passes of 8 bits.  One kernel counts the digits of all eight passes (rank_digit_hist_kernel);
// the host skips every pass whose histogram has a single non-empty bucket.  A pass is
//   rank_tile_hist_kernel  per workgroup (a tile of RK_W = 4096 consecutive keys) its 256 digit counts, LDS integer atomics: the counts do
//                          not depend on arrival order;
//   scan_*_kernel          an exclusive scan over the (digit, tile) table, digit-major: where each tile's run of each digit begins;
//   rank_scatter_kernel    the stable scatter.  A wave takes 1024 consecutive keys of the tile in 16 rounds of 64.  The rank of a key among
//                          the equal digits of its tile comes from wave order and lane order alone: within a round by eight wave64 ballots
//                          (the lanes with the same digit) and a population count of the lower lanes; across rounds by a per-wave LDS counter
//                          that the group's last lane advances with a plain store; across waves by a prefix over the four counters.  No
//                          atomic decides a position.  The tile is put into LDS in its sorted order (48 KiB) and stored from there run by
//                          run, neighbouring lanes to neighbouring addresses: stores straight from the registers, 64 lanes into up to 64
//                          runs, made the whole sort 1.7 times slower at 2^26 keys.
// Metrics.  On the sorted sequence: a tie group ends where key[i] != key[i + 1]; one inclusive integer scan of (label, group end) packed
// into 64 bits gives tp and the group number at every position; the group ends are compacted into tp[T], fp[T], threshold[T]; the terms
// of U2 (int64) and AP (fp64) are summed per workgroup in a fixed order and the workgroups' partials by one ordered reduction.
// No floating-point atomics anywhere; two runs give identical bytes.
//
// Device memory: 2 x 12 bytes per key for the two key / payload buffers, 8 for the scan, 1 for the labels, m / 2 for the tile table.
// Limits: 1 <= m < 2^31 (positions are int32; GEMHIP_E_INVALID below, GEMHIP_E_UNSUPPORTED above), refused on the host before any launch.
#include "eval_common.hpp"
#include "rank_host.hpp"
#include <algorithm>
#include <vector>

using namespace gemhip;

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_WAVES = RK_THREADS / 64;
constexpr int RK_ROUNDS = 16;                        // rounds of 64 keys per wave
constexpr int RK_W = RK_THREADS * RK_ROUNDS;         // keys per workgroup
constexpr int SC_THREADS = 256;
constexpr int SC_ITEMS = 8;
constexpr int SC_BLOCK = SC_THREADS * SC_ITEMS;      // elements per scan workgroup
constexpr int RT_ITEMS = 8;                          // tie groups per thread of rank_terms_kernel

__global__ void rank_keys_kernel(uint64_t *__restrict__ key, int32_t *__restrict__ val, int64_t m)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        key[i] = rank_key_of_bits(key[i]);
        val[i] = (int32_t)i;
    }
}

// hist [RANK_PASSES][256], zeroed by the caller.
__global__ __launch_bounds__(RK_THREADS) void rank_digit_hist_kernel(const uint64_t *__restrict__ key, int64_t m, uint32_t *__restrict__ hist)
{
    __shared__ uint32_t h[RANK_PASSES * RANK_BUCKETS];
    for (int q = threadIdx.x; q < RANK_PASSES * RANK_BUCKETS; q += RK_THREADS) h[q] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * RK_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * RK_THREADS) {
        const uint64_t k = key[i];
#pragma unroll
        for (int p = 0; p < RANK_PASSES; ++p) atomicAdd(&h[p * RANK_BUCKETS + (int)((k >> (8 * p)) & 255)], 1u);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < RANK_PASSES * RANK_BUCKETS; q += RK_THREADS)
        if (h[q]) atomicAdd(&hist[q], h[q]);
}

// tile_hist [256][ntiles]: the digit counts of tile blockIdx.x.
__global__ __launch_bounds__(RK_THREADS) void rank_tile_hist_kernel(const uint64_t *__restrict__ key, int64_t m, int shift, int64_t ntiles,
                                                                    uint64_t *__restrict__ tile_hist)
{
    __shared__ uint32_t h[RANK_BUCKETS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RK_W;
#pragma unroll 4
    for (int r = 0; r < RK_ROUNDS; ++r) {
        const int64_t i = base + r * RK_THREADS + threadIdx.x;
        if (i < m) atomicAdd(&h[(int)((key[i] >> shift) & 255)], 1u);
    }
    __syncthreads();
    tile_hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// tile_base [256][ntiles]: the exclusive scan of tile_hist.  Element e = wave * 1024 + round * 64 + lane of the tile keeps its place among the
// tile's keys of equal digit.
__global__ __launch_bounds__(RK_THREADS) void rank_scatter_kernel(const uint64_t *__restrict__ kin, const int32_t *__restrict__ vin, uint64_t *__restrict__ kout,
                                                                  int32_t *__restrict__ vout, int64_t m, int shift, int64_t ntiles,
                                                                  const uint64_t *__restrict__ tile_base)
{
    __shared__ uint32_t cnt[RK_WAVES][RANK_BUCKETS];
    __shared__ uint32_t dstart[RANK_BUCKETS];
    __shared__ long long goff[RANK_BUCKETS];
    __shared__ uint64_t skey[RK_W];                                          // 32 KiB + 16 KiB: three workgroups per CU
    __shared__ int32_t sval[RK_W];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    volatile uint32_t *mine = cnt[wave];
    for (int q = lane; q < RANK_BUCKETS; q += 64) mine[q] = 0;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * RK_W + (int64_t)wave * (64 * RK_ROUNDS) + lane;
    uint64_t key[RK_ROUNDS];
    int32_t val[RK_ROUNDS];
    uint32_t rk[RK_ROUNDS];
#pragma unroll
    for (int r = 0; r < RK_ROUNDS; ++r) {
        const int64_t i = base + r * 64;
        key[r] = i < m ? kin[i] : 0;
        val[r] = i < m ? vin[i] : 0;
    }
    const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < RK_ROUNDS; ++r) {
        const bool valid = base + r * 64 < m;
        const int digit = (int)((key[r] >> shift) & 255);
        unsigned long long same = __ballot(valid);                           // the lanes of this round whose digit is mine
#pragma unroll
        for (int b = 0; b < RANK_RADIX_BITS; ++b) {
            const bool bit = (digit >> b) & 1;
            const unsigned long long bal = __ballot(valid && bit);
            same &= bit ? bal : ~bal;
        }
        uint32_t prev = 0;
        if (valid) prev = mine[digit];                                       // what the earlier rounds of this wave counted
        rk[r] = prev + (uint32_t)__popcll(same & lower);
        if (valid && (same >> lane) == 1ull) mine[digit] = prev + (uint32_t)__popcll(same);          // the group's last lane: one plain store per digit
    }
    __syncthreads();
    uint32_t total = 0;                                                      // thread = digit: the waves' counts become their exclusive prefix
#pragma unroll
    for (int w = 0; w < RK_WAVES; ++w) {
        const uint32_t c = cnt[w][tid];
        cnt[w][tid] = total;
        total += c;
    }
    dstart[tid] = total;                                                     // ... and the digits' totals the start of each digit's run in the tile
    __syncthreads();
    for (int o = 1; o < RANK_BUCKETS; o <<= 1) {
        const uint32_t t = tid >= o ? dstart[tid - o] : 0;
        __syncthreads();
        dstart[tid] += t;
        __syncthreads();
    }
    const uint32_t first = dstart[tid] - total;
    __syncthreads();
    dstart[tid] = first;
    goff[tid] = (long long)tile_base[(size_t)tid * ntiles + blockIdx.x] - (long long)first;          // tile position -> position in the output
    __syncthreads();
    // the tile in its sorted order in LDS, then out run by run: neighbouring lanes store neighbouring addresses
#pragma unroll
    for (int r = 0; r < RK_ROUNDS; ++r) {
        if (base + r * 64 < m) {
            const int digit = (int)((key[r] >> shift) & 255);
            const uint32_t at = dstart[digit] + cnt[wave][digit] + rk[r];
            if (at < (uint32_t)RK_W) {                                       // (always: a rank among the tile's keys)
                skey[at] = key[r];
                sval[at] = val[r];
            }
        }
    }
    __syncthreads();
    const int64_t left = m - (int64_t)blockIdx.x * RK_W;
    const int here = (int)(left < RK_W ? left : RK_W);
#pragma unroll 4
    for (int r = 0; r < RK_ROUNDS; ++r) {
        const int e = r * RK_THREADS + tid;
        if (e < here) {
            const uint64_t k = skey[e];
            const long long pos = goff[(int)((k >> shift) & 255)] + e;
            if (pos >= 0 && pos < m) {                                       // (always, the table was counted from these keys)
                kout[pos] = k;
                vout[pos] = sval[e];
            }
        }
    }
}

// ---------------------------------------------------------------- scan of a uint64 array in place: block sums, their exclusive scan, apply
__global__ __launch_bounds__(SC_THREADS) void scan_sums_kernel(const uint64_t *__restrict__ a, int64_t n, uint64_t *__restrict__ bsum)
{
    __shared__ uint64_t red[SC_THREADS];
    const int64_t base = (int64_t)blockIdx.x * SC_BLOCK + (int64_t)threadIdx.x * SC_ITEMS;
    uint64_t s = 0;
#pragma unroll
    for (int j = 0; j < SC_ITEMS; ++j)
        if (base + j < n) s += a[base + j];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = SC_THREADS / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

// Inclusive scan of buf [SC_THREADS] in LDS; every thread returns its inclusive value.
__device__ __forceinline__ uint64_t scan_lds(uint64_t *buf, uint64_t v)
{
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int o = 1; o < SC_THREADS; o <<= 1) {
        const uint64_t t = tid >= o ? buf[tid - o] : 0;
        __syncthreads();
        buf[tid] += t;
        __syncthreads();
    }
    return buf[tid];
}

__global__ __launch_bounds__(SC_THREADS) void scan_bsums_kernel(uint64_t *__restrict__ bsum, int64_t nb)          // one workgroup
{
    __shared__ uint64_t buf[SC_THREADS];
    uint64_t carry = 0;                                                      // the same value in every thread
    for (int64_t start = 0; start < nb; start += SC_THREADS) {
        const int64_t i = start + threadIdx.x;
        const uint64_t v = i < nb ? bsum[i] : 0;
        const uint64_t incl = scan_lds(buf, v);
        if (i < nb) bsum[i] = carry + incl - v;
        carry += buf[SC_THREADS - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(SC_THREADS) void scan_apply_kernel(uint64_t *__restrict__ a, int64_t n, const uint64_t *__restrict__ bsum, int inclusive)
{
    __shared__ uint64_t buf[SC_THREADS];
    const int64_t base = (int64_t)blockIdx.x * SC_BLOCK + (int64_t)threadIdx.x * SC_ITEMS;
    uint64_t v[SC_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < SC_ITEMS; ++j) {
        v[j] = base + j < n ? a[base + j] : 0;
        s += v[j];
    }
    uint64_t run = scan_lds(buf, s) - s + bsum[blockIdx.x];
#pragma unroll
    for (int j = 0; j < SC_ITEMS; ++j)
        if (base + j < n) {
            a[base + j] = inclusive ? run + v[j] : run;
            run += v[j];
        }
}

// ---------------------------------------------------------------- metrics
// packed[i] = label of the i-th ranked score | (does a tie group end at i) << 32.
__global__ void rank_flags_kernel(const uint64_t *__restrict__ key, const int32_t *__restrict__ perm, const uint8_t *__restrict__ label, int64_t m,
                                  uint64_t *__restrict__ packed)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint64_t end = i == m - 1 || key[i] != key[i + 1] ? 1 : 0;
    const int64_t at = perm[i];
    const uint64_t lab = at >= 0 && at < m ? label[at] : 0;                  // (always inside: perm is a permutation)
    packed[i] = lab | (end << 32);
}

// scan[i] = tp through i | groups ended through i << 32.  Group g ends at the position that raises the count to g + 1.
__global__ void rank_groups_kernel(const uint64_t *__restrict__ key, const uint64_t *__restrict__ scan, int64_t m, int64_t T, uint32_t *__restrict__ gtp,
                                   uint32_t *__restrict__ gfp, double *__restrict__ thr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    if (!(i == m - 1 || key[i] != key[i + 1])) return;
    const int64_t g = (int64_t)(scan[i] >> 32) - 1;
    if (g < 0 || g >= T) return;                                             // (never: T is the scan's last entry)
    const uint32_t tp = (uint32_t)(scan[i] & 0xffffffffull);
    gtp[g] = tp;
    gfp[g] = (uint32_t)(i + 1) - tp;
    thr[g] = __longlong_as_double((long long)rank_bits_of_key(key[i]));
}

// Workgroup b sums the terms of groups [b * 2048, (b + 1) * 2048): a thread its eight consecutive groups in order, then a fixed tree.
__global__ __launch_bounds__(SC_THREADS) void rank_terms_kernel(const uint32_t *__restrict__ gtp, const uint32_t *__restrict__ gfp, int64_t T, int64_t N,
                                                                long long *__restrict__ partU, double *__restrict__ partAP)
{
    __shared__ long long ru[SC_THREADS];
    __shared__ double ra[SC_THREADS];
    const int64_t base = ((int64_t)blockIdx.x * SC_THREADS + threadIdx.x) * RT_ITEMS;
    long long u = 0;
    double a = 0.0;
    for (int j = 0; j < RT_ITEMS; ++j) {
        const int64_t g = base + j;
        if (g < T) {
            const int64_t tp = gtp[g], fp = gfp[g], ptp = g ? gtp[g - 1] : 0, pfp = g ? gfp[g - 1] : 0;
            u += rank_u2_term(tp - ptp, fp - pfp, fp, N);
            a += rank_ap_term(tp - ptp, tp, fp);
        }
    }
    ru[threadIdx.x] = u;
    ra[threadIdx.x] = a;
    __syncthreads();
    for (int o = SC_THREADS / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ru[threadIdx.x] += ru[threadIdx.x + o];
            ra[threadIdx.x] += ra[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partU[blockIdx.x] = ru[0];
        partAP[blockIdx.x] = ra[0];
    }
}

// One workgroup: thread t adds its contiguous share of the partials in order, thread 0 the 256 shares in order.
__global__ __launch_bounds__(SC_THREADS) void rank_final_kernel(const long long *__restrict__ partU, const double *__restrict__ partAP, int64_t nparts,
                                                                long long *__restrict__ outU, double *__restrict__ outAP)
{
    __shared__ long long ru[SC_THREADS];
    __shared__ double ra[SC_THREADS];
    const int64_t per = (nparts + SC_THREADS - 1) / SC_THREADS;
    long long u = 0;
    double a = 0.0;
    for (int64_t q = (int64_t)threadIdx.x * per; q < ((int64_t)threadIdx.x + 1) * per && q < nparts; ++q) {
        u += partU[q];
        a += partAP[q];
    }
    ru[threadIdx.x] = u;
    ra[threadIdx.x] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long su = 0;
        double sa = 0.0;
        for (int t = 0; t < SC_THREADS; ++t) { su += ru[t]; sa += ra[t]; }
        *outU = su;
        *outAP = sa;
    }
}

// ================================================================== host side

struct RankWork {
    DevBuf<uint64_t> kA, kB, packed, tile, bsum;
    DevBuf<int32_t> vA, vB;
    DevBuf<uint8_t> label;
    DevBuf<uint32_t> hist, gtp, gfp;
    DevBuf<double> thr, partAP, outAP;
    DevBuf<long long> partU, outU;
    uint64_t *keys = nullptr;            // the sorted keys and their positions: kA / vA or kB / vB
    int32_t *perm = nullptr;
    Stopwatch watch;
};

struct RankLast {
    int64_t m = 0, tiles = 0, T = 0;
    int passes = 0, skipped = 0;
    double ms = 0.0;
};
RankLast &last() { static thread_local RankLast l; return l; }

int check_scores(const char *who, int64_t m, const double *score)
{
    GEMHIP_REQUIRE(m >= 1, "%s: m = %lld (need m >= 1)", who, (long long)m);
    if (m > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "%s: m = %lld: must be below 2^31", who, (long long)m);
    GEMHIP_REQUIRE(score != nullptr, "%s: NULL score", who);
    const int64_t bad = rank_first_nan(score, m);
    GEMHIP_REQUIRE(bad < 0, "%s: score[%lld] is NaN", who, (long long)bad);
    return GEMHIP_OK;
}

// Labels in {0, 1}, both classes present; *P_out = the positives.
int check_labels(const char *who, int64_t m, const uint8_t *label, int64_t *P_out)
{
    GEMHIP_REQUIRE(label != nullptr, "%s: NULL label", who);
    const int64_t bad = rank_first_bad_label(label, m);
    GEMHIP_REQUIRE(bad < 0, "%s: label[%lld] = %d is neither 0 nor 1", who, (long long)bad, bad < 0 ? 0 : (int)label[bad]);
    int64_t P = 0;
    for (int64_t t = 0; t < m; ++t) P += label[t];
    GEMHIP_REQUIRE(P > 0, "%s: only one class present: no positive label among %lld", who, (long long)m);
    GEMHIP_REQUIRE(P < m, "%s: only one class present: no negative label among %lld", who, (long long)m);
    *P_out = P;
    return GEMHIP_OK;
}

// The kernel time of a call is the sum of its timed stretches; allocations and the copies in and out happen between them.  A stretch ends
// with a wait, which the readback or allocation that follows would make anyway.
int begin_stretch(RankWork &w)
{
    GEMHIP_CHECK(start(w.watch));
    return GEMHIP_OK;
}

int end_stretch(RankWork &w)
{
    double ms = 0.0;
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(stop(w.watch, &ms));
    last().ms += ms;
    return GEMHIP_OK;
}

int64_t scan_blocks(int64_t n) { return (n + SC_BLOCK - 1) / SC_BLOCK; }

int scan_in_place(RankWork &w, uint64_t *a, int64_t n, bool inclusive)
{
    const int64_t nb = scan_blocks(n);
    GEMHIP_CHECK(w.bsum.reserve((size_t)nb));                               // (held already: sort_scores sized it for both scans)
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nb), dim3(SC_THREADS), 0, 0, a, n, w.bsum.get());
    hipLaunchKernelGGL(scan_bsums_kernel, dim3(1), dim3(SC_THREADS), 0, 0, w.bsum.get(), nb);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nb), dim3(SC_THREADS), 0, 0, a, n, w.bsum.get(), inclusive ? 1 : 0);
    return GEMHIP_OK;
}

// Sorts; leaves w.keys / w.perm.  The inputs have been checked.
int sort_scores(RankWork &w, int64_t m, const double *score)
{
    RankLast &l = last();
    l = RankLast();
    l.m = m;
    const int64_t ntiles = (m + RK_W - 1) / RK_W;
    l.tiles = ntiles;
    GEMHIP_CHECK(w.kA.upload(reinterpret_cast<const uint64_t *>(score), (size_t)m));            // the bits of the scores, made keys in place
    GEMHIP_CHECK(w.kB.reserve((size_t)m));
    GEMHIP_CHECK(w.vA.reserve((size_t)m));
    GEMHIP_CHECK(w.vB.reserve((size_t)m));
    GEMHIP_CHECK(w.hist.reserve((size_t)RANK_PASSES * RANK_BUCKETS));
    GEMHIP_CHECK(w.tile.reserve((size_t)RANK_BUCKETS * ntiles));
    GEMHIP_CHECK(w.bsum.reserve((size_t)std::max(scan_blocks((int64_t)RANK_BUCKETS * ntiles), scan_blocks(m))));
    int rc = begin_stretch(w);
    if (rc) return rc;
    GEMHIP_CHECK(hipMemsetAsync(w.hist, 0, sizeof(uint32_t) * RANK_PASSES * RANK_BUCKETS, 0));
    const unsigned wide = grid_of(m, RK_THREADS) < 2048u ? grid_of(m, RK_THREADS) : 2048u;
    hipLaunchKernelGGL(rank_keys_kernel, dim3(wide), dim3(RK_THREADS), 0, 0, w.kA.get(), w.vA.get(), m);
    hipLaunchKernelGGL(rank_digit_hist_kernel, dim3(wide), dim3(RK_THREADS), 0, 0, w.kA.get(), m, w.hist.get());
    GEMHIP_CHECK(hipGetLastError());
    std::vector<uint32_t> hist((size_t)RANK_PASSES * RANK_BUCKETS);
    GEMHIP_CHECK(hipMemcpy(hist.data(), w.hist, hist.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    bool active[RANK_PASSES];
    l.passes = rank_active_passes(hist.data(), m, active);
    l.skipped = RANK_PASSES - l.passes;
    uint64_t *kin = w.kA, *kout = w.kB;
    int32_t *vin = w.vA, *vout = w.vB;
    for (int p = 0; p < RANK_PASSES; ++p) {
        if (!active[p]) continue;
        hipLaunchKernelGGL(rank_tile_hist_kernel, dim3((unsigned)ntiles), dim3(RK_THREADS), 0, 0, kin, m, 8 * p, ntiles, w.tile.get());
        if ((rc = scan_in_place(w, w.tile, (int64_t)RANK_BUCKETS * ntiles, false))) return rc;
        hipLaunchKernelGGL(rank_scatter_kernel, dim3((unsigned)ntiles), dim3(RK_THREADS), 0, 0, kin, vin, kout, vout, m, 8 * p, ntiles, w.tile.get());
        std::swap(kin, kout);
        std::swap(vin, vout);
    }
    w.keys = kin;
    w.perm = vin;
    return end_stretch(w);
}


// The group table of the sorted sequence on the device: w.gtp / w.gfp / w.thr [*T_out].
int group_table(RankWork &w, int64_t m, const uint8_t *label, int64_t *T_out)
{
    GEMHIP_CHECK(w.label.upload(label, (size_t)m));
    GEMHIP_CHECK(w.packed.reserve((size_t)m));
    int rc = begin_stretch(w);
    if (rc) return rc;
    hipLaunchKernelGGL(rank_flags_kernel, dim3(grid_of(m, 256)), dim3(256), 0, 0, w.keys, w.perm, w.label.get(), m, w.packed.get());
    if ((rc = scan_in_place(w, w.packed, m, true))) return rc;
    if ((rc = end_stretch(w))) return rc;
    uint64_t tail = 0;
    GEMHIP_CHECK(hipMemcpy(&tail, w.packed.get() + (m - 1), sizeof(uint64_t), hipMemcpyDeviceToHost));
    const int64_t T = (int64_t)(tail >> 32);
    if (T < 1 || T > m) return fail(GEMHIP_E_HIP, "rank: the device counted %lld tie groups among %lld scores", (long long)T, (long long)m);
    GEMHIP_CHECK(w.gtp.reserve((size_t)T));
    GEMHIP_CHECK(w.gfp.reserve((size_t)T));
    GEMHIP_CHECK(w.thr.reserve((size_t)T));
    if ((rc = begin_stretch(w))) return rc;
    hipLaunchKernelGGL(rank_groups_kernel, dim3(grid_of(m, 256)), dim3(256), 0, 0, w.keys, w.packed.get(), m, T, w.gtp.get(), w.gfp.get(), w.thr.get());
    *T_out = T;
    last().T = T;
    return end_stretch(w);
}

}  // namespace

extern "C" int gemhip_rank_argsort(int64_t m, const double *score, int32_t *perm_out)
{
    int rc = check_scores("rank_argsort", m, score);
    if (rc) return rc;
    GEMHIP_REQUIRE(perm_out != nullptr, "rank_argsort: NULL output");
    RankWork w;
    if ((rc = sort_scores(w, m, score))) return rc;
    GEMHIP_CHECK(hipMemcpy(perm_out, w.perm, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_rank_binary(int64_t m, const double *score, const uint8_t *label, double *out, int64_t *counts)
{
    int rc = check_scores("rank_binary", m, score);
    if (rc) return rc;
    int64_t P = 0, T = 0;
    if ((rc = check_labels("rank_binary", m, label, &P))) return rc;
    GEMHIP_REQUIRE(out && counts, "rank_binary: NULL output");
    const int64_t N = m - P;
    RankWork w;
    if ((rc = sort_scores(w, m, score))) return rc;
    if ((rc = group_table(w, m, label, &T))) return rc;
    const int64_t nparts = (T + SC_THREADS * RT_ITEMS - 1) / (SC_THREADS * RT_ITEMS);
    GEMHIP_CHECK(w.partU.reserve((size_t)nparts));
    GEMHIP_CHECK(w.partAP.reserve((size_t)nparts));
    GEMHIP_CHECK(w.outU.reserve(1));
    GEMHIP_CHECK(w.outAP.reserve(1));
    if ((rc = begin_stretch(w))) return rc;
    hipLaunchKernelGGL(rank_terms_kernel, dim3((unsigned)nparts), dim3(SC_THREADS), 0, 0, w.gtp.get(), w.gfp.get(), T, N, w.partU.get(), w.partAP.get());
    hipLaunchKernelGGL(rank_final_kernel, dim3(1), dim3(SC_THREADS), 0, 0, w.partU.get(), w.partAP.get(), nparts, w.outU.get(), w.outAP.get());
    if ((rc = end_stretch(w))) return rc;
    long long U2 = 0;
    double ap_sum = 0.0;
    GEMHIP_CHECK(hipMemcpy(&U2, w.outU, sizeof(U2), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(&ap_sum, w.outAP, sizeof(ap_sum), hipMemcpyDeviceToHost));
    out[0] = (double)U2 / (double)(2 * P * N);
    out[1] = ap_sum / (double)P;
    out[2] = (double)P / (double)m;
    out[3] = last().ms;
    counts[0] = P; counts[1] = N; counts[2] = T; counts[3] = (int64_t)U2;
    return GEMHIP_OK;
}

extern "C" int gemhip_rank_curve(int64_t m, const double *score, const uint8_t *label, int64_t cap, double *thr_out, int64_t *tp_out, int64_t *fp_out, int64_t *T_out)
{
    int rc = check_scores("rank_curve", m, score);
    if (rc) return rc;
    int64_t P = 0, T = 0;
    if ((rc = check_labels("rank_curve", m, label, &P))) return rc;
    GEMHIP_REQUIRE(T_out != nullptr, "rank_curve: NULL T_out");
    GEMHIP_REQUIRE(cap >= 0, "rank_curve: cap = %lld (need cap >= 0)", (long long)cap);
    RankWork w;
    if ((rc = sort_scores(w, m, score))) return rc;
    if ((rc = group_table(w, m, label, &T))) return rc;
    *T_out = T;
    if (cap < T) return fail(GEMHIP_E_INVALID, "rank_curve: %lld distinct scores, room for %lld", (long long)T, (long long)cap);
    GEMHIP_REQUIRE(thr_out && tp_out && fp_out, "rank_curve: NULL output");
    std::vector<uint32_t> tp((size_t)T), fp((size_t)T);
    GEMHIP_CHECK(hipMemcpy(tp.data(), w.gtp, (size_t)T * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(fp.data(), w.gfp, (size_t)T * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(thr_out, w.thr, (size_t)T * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t g = 0; g < T; ++g) { tp_out[g] = tp[g]; fp_out[g] = fp[g]; }
    return GEMHIP_OK;
}

extern "C" int gemhip_rank_binary_from_groups_host(int64_t T, const int64_t *tp, const int64_t *fp, double *out, int64_t *counts)
{
    GEMHIP_REQUIRE(tp && fp && out && counts, "rank_binary_from_groups_host: NULL argument");
    int64_t bad = -1;
    switch (rank_from_groups(T, tp, fp, out, counts, &bad)) {
    case RANK_OK: return GEMHIP_OK;
    case RANK_EMPTY: return fail(GEMHIP_E_INVALID, "rank_binary_from_groups_host: T = %lld (need T >= 1)", (long long)T);
    case RANK_NOT_CUMULATIVE:
        return fail(GEMHIP_E_INVALID, "rank_binary_from_groups_host: group %lld = (%lld, %lld) does not continue a cumulative table below 2^31", (long long)bad,
                    (long long)tp[bad], (long long)fp[bad]);
    case RANK_NO_POSITIVE: return fail(GEMHIP_E_INVALID, "rank_binary_from_groups_host: only one class present: no positive label");
    case RANK_NO_NEGATIVE: return fail(GEMHIP_E_INVALID, "rank_binary_from_groups_host: only one class present: no negative label");
    }
    return GEMHIP_OK;
}

extern "C" int gemhip_rank_info(int64_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "rank_info: NULL");
    const RankLast &l = last();
    out[0] = RK_W; out[1] = RK_THREADS; out[2] = RANK_RADIX_BITS; out[3] = l.passes; out[4] = l.skipped; out[5] = l.tiles; out[6] = l.T; out[7] = l.m;
    return GEMHIP_OK;
}
