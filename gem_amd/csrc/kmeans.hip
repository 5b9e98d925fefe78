// kmeans.hip -- k-means on the device: Lloyd's iteration as sklearn 1.7.2 KMeans(algorithm='lloyd') runs it on a float32
// matrix, greedy k-means++ seeding on host-supplied uniforms, and the contingency table of the labels against a caller's classes.  The host
// arithmetic (checks, centres from sums, relocation of empty clusters, draw bookkeeping, NMI / ARI / purity) is kmeans_host.hip.
//
// Kernels
//   km_assign_kernel        the score |c_k|^2 - 2 x_i . c_k of KM_ROWS rows against tiles of KM_CT centres on v_mfma_f32_32x32x2_f32, a running
//                           (score, id) minimum per row in registers -- no n x K matrix; ties to the lower cluster id.
//   km_changed_kernel       how many labels differ from the previous iteration's (integer atomic).
//   km_hist_kernel          members per (row slab, cluster), integer atomics.
//   km_slab_scan_kernel     per cluster the exclusive prefix over the slabs, and the cluster's count.
//   km_fill_kernel          the member lists as a CSR sorted by row id: a stable counting sort, no atomics.
//   km_slice_sum_kernel     the fp64 column sums of KM_SLICE consecutive members of one cluster, in a fixed shape.
//   km_slice_reduce_kernel  a cluster's slices added in slice order.
//   km_rowdist_kernel       |x_i - c_label(i)|^2 in the difference form, fp64: inertia, and the distances relocation ranks.
//   block_sum_f64_kernel    the sum of n doubles in a fixed shape (eval_common.hpp).
//   km_seed_kernel          min(D2_i, |x_i - x_cand|^2) for up to KM_MAX_TRIALS candidate rows, fp32 difference form, and the fp64 sums of
//                           every KM_SEED_BLOCK rows of it (a candidate's potential; the winner's are the next draw's cumulative blocks).
//   km_gather_rows_kernel   rows of the padded matrix by id.
//   km_contingency_kernel   table[label][class] by integer atomics.
//
// Determinism.  No floating-point atomics.  Counts are integer atomics (exact); every floating-point sum has a shape that is a function of
// n, d and the labels alone: a row's place in its cluster's member list is its rank by row id, a slice is KM_SLICE consecutive members, a
// slice's sum is 256 / cw interleaved fp64 chains added in chain order, a cluster's sum its slices in order.  Two runs give the same bytes.
//
// Limits (GEMHIP_E_UNSUPPORTED, refused on the host before any device call):
//   d        <= KM_MAX_D = 256       the KM_ROWS x (dpad + 4) float row tile of the assign kernel lives in LDS (130 KiB at d = 256)
//   K        <= KM_MAX_K = 16384     the (slab, cluster) histogram has at most KM_MAX_SLABS * K entries
//   n_trials <= KM_MAX_TRIALS = 16   km_seed_kernel keeps the candidates' rows and a block's minima in LDS
//   n        <  2^31                 row ids are int32
#include "eval_common.hpp"
#include "kmeans_host.hpp"
#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace gemhip;

struct gemhip_kmeans {
    int64_t n = 0, ld = 0;
    int d = 0, dpad = 0;
    int K = 0;                                              // of the labels on the device
    bool have_labels = false;
    double mean_var = 0.0;
    int64_t slab_rows = 0, nslabs = 0;
    DevBuf<float> Xp, Cp, cn, score, D2, cand_min, rows_out;
    DevBuf<int32_t> labels, labels_old, hist, counts, tab, member, changed, cand, gather_idx, true_lab;
    DevBuf<double> dist, scalar, slice_part, sums, seed_part;
    DevBuf<unsigned long long> table;
    Stopwatch watch;
    double ms[6] = {0, 0, 0, 0, 0, 0};                      // upload, seeding, fit, mean iteration, assign, update
    int64_t iterations = 0, relocations = 0;
};

namespace {

constexpr int KM_ROWS = 128;          // rows of X per workgroup of the assign kernel: 4 wavefronts, 32 rows each
constexpr int KM_CT = 32;             // centres per tile: one 32 x 32 MFMA result
constexpr int KM_BLOCK = 256;
constexpr int KM_STAGE = 8;           // 16-byte loads a thread has in flight while the row tile is staged
constexpr int KM_DEPTH = 8;           // (centre, row) operand pairs a lane loads ahead of their MFMAs
constexpr int KM_PAD = 4;             // floats added to the LDS row pitch: sixteen rows' 16-byte reads fall into sixteen different slots
constexpr int KM_MAX_D = 256;
constexpr int KM_MAX_K = 16384;
constexpr int KM_MAX_TRIALS = 16;
constexpr int KM_MAX_SLABS = 1024;    // row slabs of the counting sort: KM_MAX_SLABS * K histogram entries at most
constexpr int KM_SLICE = 512;         // members per slice of a cluster's sum
constexpr int KM_SUM_DEPTH = 8;       // rows a thread of the slice sum has in flight
constexpr int KM_SEED_BLOCK = 256;    // rows per block sum of the seeding
constexpr int KM_SUM_BLOCK = 1024;
constexpr int64_t KM_MAX_TABLE = (int64_t)1 << 26;          // entries of a contingency table

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

size_t km_assign_lds(int dpad) { return sizeof(float) * (size_t)KM_ROWS * (dpad + KM_PAD); }

// DEPTH (centre, row) operand pairs loaded ahead of their 4 DEPTH MFMAs, which run in column order whatever DEPTH is: the sum's bits do not
// depend on how a row's columns are grouped.  The centre reads come from L1 / L2, the row reads from LDS.
template <int DEPTH>
__device__ __forceinline__ void km_mfma_group(const f32x4 *__restrict__ pa, const f32x4 *pb, f32x16 &acc)
{
    f32x4 a[DEPTH], b[DEPTH];
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) { a[u] = pa[u]; b[u] = pb[u]; }
    __builtin_amdgcn_sched_barrier(0);                                   // (the scheduler otherwise sinks every load to its MFMA to save registers)
#pragma unroll
    for (int u = 0; u < DEPTH; ++u) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].x, b[u].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].y, b[u].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].z, b[u].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].w, b[u].w, acc, 0, 0, 0);
    }
}

// Workgroup b owns rows [KM_ROWS b, KM_ROWS b + KM_ROWS), staged once into LDS (rows past n repeat row n - 1 and are not written back);
// wavefront w owns 32 of them against every centre tile.  MFMA 32x32x2 computes D[i][j] = sum_k A[i][k] B[k][j] with lane l supplying
// A[l & 31][l >> 5] and B[l >> 5][l & 31] and holding D[(q & 3) + 8 (q >> 2) + 4 (l >> 5)][l & 31] in register q.  A = the centre tile,
// B = the rows: a lane then holds ONE row's products with 16 centres, and the running minimum needs no traffic between lanes until the two
// lane halves are merged at the end.  Which two of the dpad products the halves supply per instruction is free as long as A and B agree:
// half h walks columns [h dpad / 2, (h + 1) dpad / 2) with 16-byte loads.  A lane meets its centres in ascending id and replaces its best on
// a strictly smaller score only; the merge prefers the lower id on equal scores: ties go to the lower cluster id.
// Cp [ktiles * KM_CT][dpad], cn [ktiles * KM_CT] with +inf for the padding centres (their score is +inf: never strictly smaller).
__global__ __launch_bounds__(KM_BLOCK) void km_assign_kernel(const float *__restrict__ Xp, int64_t n, int dpad, const float *__restrict__ Cp,
                                                              const float *__restrict__ cn, int ktiles, int32_t *__restrict__ labels,
                                                              float *__restrict__ score_out)
{
    extern __shared__ __attribute__((aligned(16))) float km_xs[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, l31 = lane & 31;
    const int64_t row0 = (int64_t)blockIdx.x * KM_ROWS;
    const int pitch = dpad + KM_PAD, nq4 = dpad >> 2, half = dpad >> 1, nq = half >> 2;
    {
        const f32x4 *src = reinterpret_cast<const f32x4 *>(Xp);
        f32x4 *dst = reinterpret_cast<f32x4 *>(km_xs);
        for (int e0 = tid; e0 < KM_ROWS * nq4; e0 += KM_BLOCK * KM_STAGE) {          // KM_STAGE loads in flight per thread, then their stores
            f32x4 v[KM_STAGE];
#pragma unroll
            for (int u = 0; u < KM_STAGE; ++u) {
                const int e = e0 + u * KM_BLOCK;
                if (e < KM_ROWS * nq4) {
                    const int r = e / nq4, q = e - r * nq4;
                    const int64_t gr = row0 + r < n ? row0 + r : n - 1;
                    v[u] = src[gr * nq4 + q];
                }
            }
#pragma unroll
            for (int u = 0; u < KM_STAGE; ++u) {
                const int e = e0 + u * KM_BLOCK;
                if (e < KM_ROWS * nq4) {
                    const int r = e / nq4, q = e - r * nq4;
                    dst[r * (pitch >> 2) + q] = v[u];
                }
            }
        }
    }
    __syncthreads();
    const f32x4 *pb = reinterpret_cast<const f32x4 *>(km_xs + (wave * 32 + l31) * pitch + h * half);
    float best = INFINITY;
    int32_t best_id = 0;
    for (int ct = 0; ct < ktiles; ++ct) {
        const f32x4 *pa = reinterpret_cast<const f32x4 *>(Cp + ((int64_t)ct * KM_CT + l31) * dpad + h * half);
        f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.f;
        int t = 0;
        for (; t + KM_DEPTH <= nq; t += KM_DEPTH) km_mfma_group<KM_DEPTH>(pa + t, pb + t, acc);
        if (t + 4 <= nq) { km_mfma_group<4>(pa + t, pb + t, acc); t += 4; }
        if (t + 2 <= nq) { km_mfma_group<2>(pa + t, pb + t, acc); t += 2; }
        if (t < nq) km_mfma_group<1>(pa + t, pb + t, acc);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int id = ct * KM_CT + (q & 3) + 8 * (q >> 2) + 4 * h;          // ascending in q
            const float s = fmaf(-2.f, acc[q], cn[id]);
            if (s < best) { best = s; best_id = id; }
        }
    }
    const float other = __shfl_xor(best, 32);
    const int32_t other_id = __shfl_xor(best_id, 32);
    if (other < best || (other == best && other_id < best_id)) { best = other; best_id = other_id; }
    const int64_t gi = row0 + wave * 32 + l31;
    if (h == 0 && gi < n) {
        labels[gi] = best_id;
        if (score_out) score_out[gi] = best;
    }
}

__global__ __launch_bounds__(256) void km_changed_kernel(const int32_t *__restrict__ a, const int32_t *__restrict__ b, int64_t n, int32_t *changed)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && a[i] != b[i]) atomicAdd(changed, 1);
}

// hist [nslabs][K]: slab s = rows [s slab_rows, (s + 1) slab_rows).
__global__ __launch_bounds__(256) void km_hist_kernel(const int32_t *__restrict__ labels, int64_t n, int64_t slab_rows, int K, int32_t *hist)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(hist + (i / slab_rows) * K + labels[i], 1);
}

// hist[s][k] becomes the number of members of cluster k in the slabs before s; counts[k] the cluster's size.  One wavefront per cluster,
// 64 slabs per step: an inclusive scan across the lanes and a running carry (integers: exact).
__global__ __launch_bounds__(256) void km_slab_scan_kernel(int32_t *__restrict__ hist, int64_t nslabs, int K, int32_t *__restrict__ counts)
{
    const int lane = lane_id();
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;                                                   // (the same in all lanes)
    int32_t carry = 0;
    for (int64_t base = 0; base < nslabs; base += WAVE) {
        const int64_t s = base + lane;
        const int32_t c = s < nslabs ? hist[s * K + k] : 0;
        int32_t incl = c;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int32_t o = __shfl_up(incl, off);
            if (lane >= off) incl += o;
        }
        if (s < nslabs) hist[s * K + k] = carry + incl - c;
        carry += __shfl(incl, WAVE - 1);
    }
    if (lane == 0) counts[k] = carry;
}

// One workgroup per slab, 256 rows at a time in row order: a row's slot is ptr[label] + (members in earlier slabs) + (members earlier in this
// slab), the last counted by comparing the 256 labels in LDS.  cursor = hist after km_slab_scan_kernel; the slab's own entries advance.
__global__ __launch_bounds__(256) void km_fill_kernel(const int32_t *__restrict__ labels, int64_t n, int64_t slab_rows, int K, volatile int32_t *cursor,
                                                       const int32_t *__restrict__ ptr, int32_t *__restrict__ member)
{
    __shared__ int32_t lab[256];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * slab_rows;
    const int64_t r1 = r0 + slab_rows < n ? r0 + slab_rows : n;
    volatile int32_t *cur = cursor + (int64_t)blockIdx.x * K;
    for (int64_t base = r0; base < r1; base += 256) {
        const int64_t i = base + tid;
        const int32_t l = i < r1 ? labels[i] : -1;
        lab[tid] = l;
        __syncthreads();
        int rank = 0, total = 0;
        if (l >= 0) {
            for (int j = 0; j < 256; ++j) {
                const int m = lab[j] == l ? 1 : 0;
                rank += j < tid ? m : 0;
                total += m;
            }
            member[ptr[l] + cur[l] + rank] = (int32_t)i;
        }
        __syncthreads();                                                  // every read of the cursor is through
        if (l >= 0 && rank == total - 1) cur[l] = cur[l] + total;          // the last row of its label in these 256: one writer per entry
        __syncthreads();
    }
}

// Slice s: members [begin[s], begin[s] + len[s]) of one cluster.  Thread (g, c) adds column c of members g, g + G, ... in that order
// (G = 256 / cw chains, cw the power of two >= dpad); the chains are then added in chain order.  part [nslices][dpad].
__global__ __launch_bounds__(256) void km_slice_sum_kernel(const float *__restrict__ Xp, int dpad, int cw, const int32_t *__restrict__ member,
                                                            const int32_t *__restrict__ begin, const int32_t *__restrict__ len, double *__restrict__ part)
{
    __shared__ double red[256];
    const int tid = threadIdx.x, c = tid & (cw - 1), g = tid / cw, G = 256 / cw;
    const int32_t b = begin[blockIdx.x], L = len[blockIdx.x];
    double acc = 0.0;
    if (c < dpad) {
        int32_t m = g;
        for (; m + (KM_SUM_DEPTH - 1) * G < L; m += KM_SUM_DEPTH * G) {          // KM_SUM_DEPTH rows in flight, added in the order of the plain loop
            int32_t id[KM_SUM_DEPTH];
            float v[KM_SUM_DEPTH];
#pragma unroll
            for (int u = 0; u < KM_SUM_DEPTH; ++u) id[u] = member[b + m + u * G];
#pragma unroll
            for (int u = 0; u < KM_SUM_DEPTH; ++u) v[u] = Xp[(int64_t)id[u] * dpad + c];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < KM_SUM_DEPTH; ++u) acc += (double)v[u];
        }
        for (; m < L; m += G) acc += (double)Xp[(int64_t)member[b + m] * dpad + c];
    }
    red[tid] = acc;
    __syncthreads();
    if (g == 0 && c < dpad) {
        double s = 0.0;
        for (int gg = 0; gg < G; ++gg) s += red[gg * cw + c];
        part[(int64_t)blockIdx.x * dpad + c] = s;
    }
}

// sums[k][c] = the slices slice_ptr[k] .. slice_ptr[k + 1] of cluster k in order.
__global__ __launch_bounds__(256) void km_slice_reduce_kernel(const double *__restrict__ part, const int32_t *__restrict__ slice_ptr, int K, int dpad,
                                                               double *__restrict__ sums)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)K * dpad) return;
    const int k = (int)(q / dpad), c = (int)(q - (int64_t)k * dpad);
    double s = 0.0;
    for (int32_t t = slice_ptr[k]; t < slice_ptr[k + 1]; ++t) s += part[(int64_t)t * dpad + c];
    sums[q] = s;
}

// dist[i] = sum_c (x_ic - centre[label_i][c])^2, fp64: one wavefront per row, a lane's columns in order, then the butterfly.
__global__ __launch_bounds__(256) void km_rowdist_kernel(const float *__restrict__ Xp, int64_t n, int dpad, const float *__restrict__ Cp,
                                                          const int32_t *__restrict__ labels, double *__restrict__ dist)
{
    const int lane = lane_id();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float *x = Xp + i * dpad, *cc = Cp + (int64_t)labels[i] * dpad;
    double s = 0.0;
    for (int c = lane; c < dpad; c += WAVE) {
        const double t = (double)x[c] - (double)cc[c];
        s = fma(t, t, s);
    }
    s = wave_sum_f64(s);
    if (lane == 0) dist[i] = s;
}

// Workgroup b: rows [256 b, 256 b + 256), wavefront w rows w, w + 4, ...  For candidate t < T (row cand[t]):
//     out_min[t][i] = min(D2[i], |x_i - x_cand|^2)    (D2 == nullptr: the distance itself), fp32, the difference form;
//     part[t][b]    = the fp64 sum of the block's 256 values: lane l adds rows 4 l .. 4 l + 3 in order, then the butterfly.
__global__ __launch_bounds__(256) void km_seed_kernel(const float *__restrict__ Xp, int64_t n, int dpad, const int32_t *__restrict__ cand, int T,
                                                       const float *__restrict__ D2, float *__restrict__ out_min, double *__restrict__ part, int64_t nb)
{
    __shared__ float cs[KM_MAX_TRIALS][KM_MAX_D];
    __shared__ float mins[KM_MAX_TRIALS][KM_SEED_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < T * dpad; e += 256) {
        const int t = e / dpad, c = e - t * dpad;
        cs[t][c] = Xp[(int64_t)cand[t] * dpad + c];
    }
    __syncthreads();
    const int64_t row0 = (int64_t)blockIdx.x * KM_SEED_BLOCK;
    for (int r = wave; r < KM_SEED_BLOCK; r += 4) {
        const int64_t i = row0 + r;
        if (i >= n) {                                                     // (the same in all lanes)
            if (lane < T) mins[lane][r] = 0.f;
            continue;
        }
        float xv[KM_MAX_D / WAVE];
#pragma unroll
        for (int j = 0; j < KM_MAX_D / WAVE; ++j) xv[j] = lane + WAVE * j < dpad ? Xp[i * dpad + lane + WAVE * j] : 0.f;
        const float old = D2 ? D2[i] : INFINITY;
        for (int t = 0; t < T; ++t) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KM_MAX_D / WAVE; ++j) {
                const float df = lane + WAVE * j < dpad ? xv[j] - cs[t][lane + WAVE * j] : 0.f;
                s = fmaf(df, df, s);
            }
            s = wave_sum(s);
            const float m = s < old ? s : old;
            if (lane == 0) {
                mins[t][r] = m;
                out_min[(int64_t)t * n + i] = m;
            }
        }
    }
    __syncthreads();
    for (int t = wave; t < T; t += 4) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += (double)mins[t][lane * 4 + j];
        s = wave_sum_f64(s);
        if (lane == 0) part[(int64_t)t * nb + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void km_gather_rows_kernel(const float *__restrict__ Xp, int dpad, const int32_t *__restrict__ idx, int64_t m,
                                                              float *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m * dpad) return;
    const int64_t r = q / dpad;
    out[q] = Xp[(int64_t)idx[r] * dpad + (q - r * dpad)];
}

__global__ __launch_bounds__(256) void km_contingency_kernel(const int32_t *__restrict__ labels, const int32_t *__restrict__ truth, int64_t n, int Kt,
                                                              unsigned long long *table)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(table + (int64_t)labels[i] * Kt + truth[i], 1ull);
}

// ================================================================== host side
int check_K(const char *who, const gemhip_kmeans *h, int32_t K)
{
    GEMHIP_REQUIRE(h != nullptr, "%s: NULL handle", who);
    GEMHIP_REQUIRE(K >= 1, "%s: K = %d (need K >= 1)", who, K);
    GEMHIP_REQUIRE((int64_t)K <= h->n, "%s: K = %d exceeds n = %lld", who, K, (long long)h->n);
    if (K > KM_MAX_K) return fail(GEMHIP_E_UNSUPPORTED, "%s: K = %d: at most %d clusters", who, K, KM_MAX_K);
    return GEMHIP_OK;
}

int check_centres(const char *who, int32_t K, int32_t d, const float *C)
{
    GEMHIP_REQUIRE(C != nullptr, "%s: NULL centres", who);
    for (int32_t k = 0; k < K; ++k)
        for (int32_t c = 0; c < d; ++c) GEMHIP_REQUIRE(std::isfinite(C[(size_t)k * d + c]), "%s: centre[%d][%d] is not finite", who, k, c);
    return GEMHIP_OK;
}

// C [K][d] to the device as the padded block the kernels read.
int upload_centres(gemhip_kmeans *h, int32_t K, const float *C)
{
    const int Kp = (K + KM_CT - 1) / KM_CT * KM_CT;
    std::vector<float> cp((size_t)Kp * h->dpad), cn((size_t)Kp);
    km_pad_centres(K, h->d, h->dpad, Kp, C, cp.data(), cn.data());
    GEMHIP_CHECK(h->Cp.upload(cp.data(), cp.size()));
    GEMHIP_CHECK(h->cn.upload(cn.data(), cn.size()));
    return GEMHIP_OK;
}

// Labels of all rows against the centres upload_centres put there, into h->labels (and h->score).
int enqueue_assign(gemhip_kmeans *h, int32_t K, bool want_score)
{
    GEMHIP_CHECK(h->labels.reserve((size_t)h->n));
    if (want_score) GEMHIP_CHECK(h->score.reserve((size_t)h->n));
    hipLaunchKernelGGL(km_assign_kernel, dim3(grid_of(h->n, KM_ROWS)), dim3(KM_BLOCK), km_assign_lds(h->dpad), 0, h->Xp.get(), h->n, h->dpad, h->Cp.get(),
                       h->cn.get(), (K + KM_CT - 1) / KM_CT, h->labels.get(), want_score ? h->score.get() : (float *)nullptr);
    GEMHIP_CHECK(hipGetLastError());
    h->K = K;
    h->have_labels = true;
    return GEMHIP_OK;
}

// The update of h->labels (K clusters): counts [K] and the fp64 sums [K][dpad] on the host.
int run_update(gemhip_kmeans *h, int32_t K, std::vector<double> &sums, std::vector<int64_t> &counts)
{
    const int64_t n = h->n;
    const int dpad = h->dpad;
    GEMHIP_CHECK(h->hist.reserve((size_t)h->nslabs * K));
    GEMHIP_CHECK(h->counts.reserve((size_t)K));
    GEMHIP_CHECK(h->member.reserve((size_t)n));
    GEMHIP_CHECK(hipMemsetAsync(h->hist, 0, (size_t)h->nslabs * K * sizeof(int32_t), 0));
    hipLaunchKernelGGL(km_hist_kernel, dim3(grid_of(n, 256)), dim3(256), 0, 0, h->labels.get(), n, h->slab_rows, K, h->hist.get());
    hipLaunchKernelGGL(km_slab_scan_kernel, dim3(grid_of(K, 4)), dim3(256), 0, 0, h->hist.get(), h->nslabs, K, h->counts.get());
    GEMHIP_CHECK(hipGetLastError());
    std::vector<int32_t> cnt((size_t)K);
    GEMHIP_CHECK(hipMemcpy(cnt.data(), h->counts, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost));
    // tab = ptr [K + 1], slice_ptr [K + 1], begin [nslices], len [nslices]
    std::vector<int32_t> tab((size_t)2 * (K + 1));
    std::vector<int32_t> begin, len;
    int64_t total = 0;
    for (int32_t k = 0; k < K; ++k) {
        tab[k] = (int32_t)total;
        tab[(size_t)K + 1 + k] = (int32_t)begin.size();
        for (int32_t o = 0; o < cnt[k]; o += KM_SLICE) {
            begin.push_back((int32_t)total + o);
            len.push_back(cnt[k] - o < KM_SLICE ? cnt[k] - o : KM_SLICE);
        }
        total += cnt[k];
    }
    if (total != n) return fail(GEMHIP_E_HIP, "kmeans update: the cluster counts add up to %lld, not n = %lld", (long long)total, (long long)n);
    tab[K] = (int32_t)total;
    tab[(size_t)2 * K + 1] = (int32_t)begin.size();
    const size_t nslices = begin.size();
    tab.insert(tab.end(), begin.begin(), begin.end());
    tab.insert(tab.end(), len.begin(), len.end());
    GEMHIP_CHECK(h->tab.upload(tab.data(), tab.size()));
    GEMHIP_CHECK(h->slice_part.reserve(nslices * dpad));
    GEMHIP_CHECK(h->sums.reserve((size_t)K * dpad));
    const int32_t *ptr = h->tab.get(), *slice_ptr = ptr + K + 1, *d_begin = slice_ptr + K + 1, *d_len = d_begin + nslices;
    int cw = 8;
    while (cw < dpad) cw *= 2;
    hipLaunchKernelGGL(km_fill_kernel, dim3((unsigned)h->nslabs), dim3(256), 0, 0, h->labels.get(), n, h->slab_rows, K, h->hist.get(), ptr, h->member.get());
    hipLaunchKernelGGL(km_slice_sum_kernel, dim3((unsigned)nslices), dim3(256), 0, 0, h->Xp.get(), dpad, cw, h->member.get(), d_begin, d_len, h->slice_part.get());
    hipLaunchKernelGGL(km_slice_reduce_kernel, dim3(grid_of((int64_t)K * dpad, 256)), dim3(256), 0, 0, h->slice_part.get(), slice_ptr, K, dpad, h->sums.get());
    GEMHIP_CHECK(hipGetLastError());
    sums.resize((size_t)K * dpad);
    GEMHIP_CHECK(hipMemcpy(sums.data(), h->sums, sums.size() * sizeof(double), hipMemcpyDeviceToHost));
    counts.assign(cnt.begin(), cnt.end());
    return GEMHIP_OK;
}

// dist[i] of h->labels against the centre block on the device, into h->dist.
int enqueue_rowdist(gemhip_kmeans *h)
{
    GEMHIP_CHECK(h->dist.reserve((size_t)h->n));
    hipLaunchKernelGGL(km_rowdist_kernel, dim3(grid_of(h->n, 4)), dim3(256), 0, 0, h->Xp.get(), h->n, h->dpad, h->Cp.get(), h->labels.get(), h->dist.get());
    GEMHIP_CHECK(hipGetLastError());
    return GEMHIP_OK;
}

// out [m][dpad] = rows idx [m] of the padded matrix.
int gather_rows(gemhip_kmeans *h, const std::vector<int32_t> &idx, std::vector<float> &out)
{
    const int64_t m = (int64_t)idx.size();
    out.resize((size_t)m * h->dpad);
    if (!m) return GEMHIP_OK;
    GEMHIP_CHECK(h->gather_idx.upload(idx.data(), idx.size()));
    GEMHIP_CHECK(h->rows_out.reserve(out.size()));
    hipLaunchKernelGGL(km_gather_rows_kernel, dim3(grid_of(m * h->dpad, 256)), dim3(256), 0, 0, h->Xp.get(), h->dpad, h->gather_idx.get(), m, h->rows_out.get());
    GEMHIP_CHECK(hipGetLastError());
    GEMHIP_CHECK(hipMemcpy(out.data(), h->rows_out, out.size() * sizeof(float), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

// sklearn's _relocate_empty_clusters_dense on an update's sums and counts; the centre block on the device still holds the OLD centres.
int relocate_empty(gemhip_kmeans *h, int32_t K, std::vector<double> &sums, std::vector<int64_t> &counts, int64_t *moved)
{
    std::vector<int32_t> empty;
    for (int32_t k = 0; k < K; ++k)
        if (counts[k] == 0) empty.push_back(k);
    *moved = (int64_t)empty.size();
    if (empty.empty()) return GEMHIP_OK;
    int rc = enqueue_rowdist(h);
    if (rc) return rc;
    std::vector<double> dist((size_t)h->n);
    std::vector<int32_t> lab((size_t)h->n);
    GEMHIP_CHECK(hipMemcpy(dist.data(), h->dist, dist.size() * sizeof(double), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(lab.data(), h->labels, lab.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> far(empty.size());
    km_relocation_order(h->n, dist.data(), (int64_t)empty.size(), far.data());
    std::vector<int32_t> rows(empty.size()), donor(empty.size());
    for (size_t j = 0; j < empty.size(); ++j) { rows[j] = (int32_t)far[j]; donor[j] = lab[far[j]]; }
    std::vector<float> xrows;
    if ((rc = gather_rows(h, rows, xrows))) return rc;
    const int64_t bad = km_relocate(K, h->dpad, empty, donor.data(), xrows.data(), sums.data(), counts.data());
    if (bad >= 0)
        return fail(GEMHIP_E_UNSUPPORTED, "kmeans fit: moving row %d into the empty cluster %d would leave its cluster %d without a row", rows[bad], empty[bad],
                    donor[bad]);
    return GEMHIP_OK;
}

}  // namespace

extern "C" int gemhip_kmeans_create(int64_t n, int32_t d, int32_t ld, const float *X_host, gemhip_kmeans_t *out)
{
    GEMHIP_REQUIRE(out != nullptr, "kmeans_create: NULL output");
    *out = nullptr;
    const int rc = check_embedding("kmeans_create", n, d, ld, X_host, 1, KM_MAX_D, "the LDS row tile of the assign kernel");
    if (rc) return rc;
    const int64_t bad = first_bad_entry(X_host, n, d, ld, INFINITY);
    GEMHIP_REQUIRE(bad < 0, "kmeans_create: X[%lld][%d] is not finite", (long long)(bad / d), (int)(bad % d));
    std::unique_ptr<gemhip_kmeans> h(new gemhip_kmeans);
    h->n = n; h->ld = ld; h->d = d; h->dpad = (d + 7) & ~7;
    h->slab_rows = ((n + KM_MAX_SLABS - 1) / KM_MAX_SLABS + 255) / 256 * 256;
    h->nslabs = (n + h->slab_rows - 1) / h->slab_rows;
    h->mean_var = km_mean_variance(X_host, n, d, ld);
    std::vector<float> xp((size_t)n * h->dpad);
    pad_rows(X_host, n, d, ld, h->dpad, xp.data());
    const double t0 = wall_ms();
    GEMHIP_CHECK(h->Xp.upload(xp.data(), xp.size()));
    GEMHIP_CHECK(hipDeviceSynchronize());
    h->ms[0] = wall_ms() - t0;
    GEMHIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(km_assign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)km_assign_lds(KM_MAX_D)));
    *out = h.release();
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_destroy(gemhip_kmeans_t h)
{
    delete h;
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_assign(gemhip_kmeans_t h, int32_t K, const float *centres, int32_t *labels_out, float *score_out_or_null)
{
    int rc = check_K("kmeans_assign", h, K);
    if (rc) return rc;
    if ((rc = check_centres("kmeans_assign", K, h->d, centres))) return rc;
    GEMHIP_REQUIRE(labels_out != nullptr, "kmeans_assign: NULL output");
    if ((rc = upload_centres(h, K, centres))) return rc;
    GEMHIP_CHECK(start(h->watch));
    if ((rc = enqueue_assign(h, K, score_out_or_null != nullptr))) return rc;
    GEMHIP_CHECK(stop(h->watch, &h->ms[4]));
    GEMHIP_CHECK(hipMemcpy(labels_out, h->labels, (size_t)h->n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (score_out_or_null) GEMHIP_CHECK(hipMemcpy(score_out_or_null, h->score, (size_t)h->n * sizeof(float), hipMemcpyDeviceToHost));
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_update(gemhip_kmeans_t h, int32_t K, const int32_t *labels, float *centres_out, int64_t *counts_out)
{
    int rc = check_K("kmeans_update", h, K);
    if (rc) return rc;
    GEMHIP_REQUIRE(labels && centres_out && counts_out, "kmeans_update: NULL argument");
    const int64_t bad = first_bad_index(labels, h->n, K);
    GEMHIP_REQUIRE(bad < 0, "kmeans_update: label %lld = %d outside [0,%d)", (long long)bad, labels[bad], K);
    GEMHIP_CHECK(h->labels.upload(labels, (size_t)h->n));
    h->K = K;
    h->have_labels = true;
    std::vector<double> sums;
    std::vector<int64_t> counts;
    GEMHIP_CHECK(start(h->watch));
    if ((rc = run_update(h, K, sums, counts))) return rc;
    GEMHIP_CHECK(stop(h->watch, &h->ms[5]));
    km_centres_from_sums(K, h->d, h->dpad, sums.data(), counts.data(), centres_out);
    for (int32_t k = 0; k < K; ++k) counts_out[k] = counts[k];
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_fit(gemhip_kmeans_t h, int32_t K, float *centres_inout, double tol, int32_t max_iter, int32_t *labels_out, double *info_out)
{
    int rc = check_K("kmeans_fit", h, K);
    if (rc) return rc;
    GEMHIP_REQUIRE(max_iter >= 1, "kmeans_fit: max_iter = %d (need >= 1)", max_iter);
    GEMHIP_REQUIRE(tol >= 0.0 && std::isfinite(tol), "kmeans_fit: tol = %g (need a finite tol >= 0)", tol);
    if ((rc = check_centres("kmeans_fit", K, h->d, centres_inout))) return rc;
    GEMHIP_REQUIRE(labels_out != nullptr, "kmeans_fit: NULL output");
    const int64_t n = h->n;
    const int d = h->d;
    const double tol_abs = tol * h->mean_var;
    std::vector<float> C(centres_inout, centres_inout + (size_t)K * d), Cnew((size_t)K * d);
    std::vector<double> sums;
    std::vector<int64_t> counts;
    GEMHIP_CHECK(h->labels_old.reserve((size_t)n));
    GEMHIP_CHECK(h->changed.reserve(1));
    GEMHIP_CHECK(hipMemsetAsync(h->labels_old, 0xFF, (size_t)n * sizeof(int32_t), 0));          // -1: no label equals it
    bool strict = false;
    double shift = 0.0;
    h->iterations = 0; h->relocations = 0;
    GEMHIP_CHECK(start(h->watch));
    for (int it = 0; it < max_iter; ++it) {
        if ((rc = upload_centres(h, K, C.data()))) return rc;
        if ((rc = enqueue_assign(h, K, false))) return rc;
        GEMHIP_CHECK(hipMemsetAsync(h->changed, 0, sizeof(int32_t), 0));
        hipLaunchKernelGGL(km_changed_kernel, dim3(grid_of(n, 256)), dim3(256), 0, 0, h->labels.get(), h->labels_old.get(), n, h->changed.get());
        if ((rc = run_update(h, K, sums, counts))) return rc;
        int64_t moved = 0;
        if ((rc = relocate_empty(h, K, sums, counts, &moved))) return rc;
        h->relocations += moved;
        km_centres_from_sums(K, d, h->dpad, sums.data(), counts.data(), Cnew.data());
        int32_t changed = 0;
        GEMHIP_CHECK(hipMemcpy(&changed, h->changed, sizeof(int32_t), hipMemcpyDeviceToHost));
        shift = km_centre_shift(K, d, Cnew.data(), C.data());
        C.swap(Cnew);
        h->iterations = it + 1;
        if (changed == 0) { strict = true; break; }
        if (shift <= tol_abs) break;
        GEMHIP_CHECK(hipMemcpyAsync(h->labels_old, h->labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, 0));
    }
    if ((rc = upload_centres(h, K, C.data()))) return rc;
    if (!strict && (rc = enqueue_assign(h, K, false))) return rc;                   // labels that belong to the returned centres
    GEMHIP_CHECK(stop(h->watch, &h->ms[2]));
    h->ms[3] = h->ms[2] / (double)h->iterations;
    if ((rc = enqueue_rowdist(h))) return rc;
    GEMHIP_CHECK(h->scalar.reserve(1));
    hipLaunchKernelGGL((block_sum_f64_kernel<KM_SUM_BLOCK, gemhip_kmeans>), dim3(1), dim3(KM_SUM_BLOCK), 0, 0, h->dist.get(), n, h->scalar.get());
    GEMHIP_CHECK(hipGetLastError());
    double inertia = 0.0;
    GEMHIP_CHECK(hipMemcpy(&inertia, h->scalar, sizeof(double), hipMemcpyDeviceToHost));
    GEMHIP_CHECK(hipMemcpy(labels_out, h->labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < C.size(); ++q) centres_inout[q] = C[q];
    if (info_out) {
        info_out[0] = inertia; info_out[1] = (double)h->iterations; info_out[2] = strict ? 1.0 : 0.0; info_out[3] = (double)h->relocations;
        info_out[4] = shift; info_out[5] = tol_abs;
    }
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_seed_pp(gemhip_kmeans_t h, int32_t K, int32_t n_trials, const double *u, int32_t *chosen_idx_out, float *centres_out)
{
    int rc = check_K("kmeans_seed_pp", h, K);
    if (rc) return rc;
    GEMHIP_REQUIRE(n_trials >= 1, "kmeans_seed_pp: n_trials = %d (need >= 1)", n_trials);
    if (n_trials > KM_MAX_TRIALS) return fail(GEMHIP_E_UNSUPPORTED, "kmeans_seed_pp: n_trials = %d: at most %d", n_trials, KM_MAX_TRIALS);
    GEMHIP_REQUIRE(u && chosen_idx_out && centres_out, "kmeans_seed_pp: NULL argument");
    const int64_t badu = km_first_bad_uniform(u, (int64_t)K * n_trials);
    GEMHIP_REQUIRE(badu < 0, "kmeans_seed_pp: u[%lld][%d] = %g outside [0,1)", (long long)(badu / n_trials), (int)(badu % n_trials), u[badu]);
    const int64_t n = h->n, nb = (n + KM_SEED_BLOCK - 1) / KM_SEED_BLOCK;
    const double t0 = wall_ms();
    GEMHIP_CHECK(h->D2.reserve((size_t)n));
    GEMHIP_CHECK(h->cand_min.reserve((size_t)n * n_trials));
    GEMHIP_CHECK(h->seed_part.reserve((size_t)nb * n_trials));
    GEMHIP_CHECK(h->cand.reserve((size_t)n_trials));
    std::vector<double> part((size_t)nb * n_trials), prefix((size_t)nb + 1, 0.0);
    std::vector<int32_t> cand((size_t)n_trials), chosen;
    std::vector<float> block((size_t)KM_SEED_BLOCK);
    for (int32_t c = 0; c < K; ++c) {
        int T = 1;
        if (c == 0) cand[0] = (int32_t)km_first_row(u[0], n);
        else {
            T = n_trials;
            const double total = prefix[nb];
            for (int t = 0; t < T; ++t) {
                const double v = u[(size_t)c * n_trials + t] * total;
                int64_t row = n - 1;                                       // searchsorted past the end, clipped
                for (int64_t b = km_find_block(prefix.data(), nb, v); b < nb; ++b) {
                    const int64_t first = b * KM_SEED_BLOCK, len = first + KM_SEED_BLOCK < n ? KM_SEED_BLOCK : n - first;
                    GEMHIP_CHECK(hipMemcpy(block.data(), h->D2.get() + first, (size_t)len * sizeof(float), hipMemcpyDeviceToHost));
                    const int64_t at = km_find_in_block(prefix[b], block.data(), len, v);
                    if (at >= 0) { row = first + at; break; }
                }
                cand[t] = (int32_t)row;
            }
        }
        GEMHIP_CHECK(hipMemcpy(h->cand, cand.data(), (size_t)T * sizeof(int32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(km_seed_kernel, dim3((unsigned)nb), dim3(256), 0, 0, h->Xp.get(), n, h->dpad, h->cand.get(), T,
                           c == 0 ? (const float *)nullptr : h->D2.get(), h->cand_min.get(), h->seed_part.get(), nb);
        GEMHIP_CHECK(hipGetLastError());
        GEMHIP_CHECK(hipMemcpy(part.data(), h->seed_part, (size_t)nb * T * sizeof(double), hipMemcpyDeviceToHost));
        int best = 0;
        double best_pot = 0.0;
        for (int t = 0; t < T; ++t) {
            double pot = 0.0;
            for (int64_t b = 0; b < nb; ++b) pot += part[(size_t)t * nb + b];
            if (t == 0 || pot < best_pot) { best = t; best_pot = pot; }
        }
        for (int64_t b = 0; b < nb; ++b) prefix[b + 1] = prefix[b] + part[(size_t)best * nb + b];
        GEMHIP_CHECK(hipMemcpy(h->D2, h->cand_min.get() + (size_t)best * n, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice));
        chosen.push_back(cand[best]);
    }
    std::vector<float> rows;
    if ((rc = gather_rows(h, chosen, rows))) return rc;
    for (int32_t k = 0; k < K; ++k) {
        chosen_idx_out[k] = chosen[k];
        for (int c = 0; c < h->d; ++c) centres_out[(size_t)k * h->d + c] = rows[(size_t)k * h->dpad + c];
    }
    h->ms[1] = wall_ms() - t0;
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_contingency(gemhip_kmeans_t h, int32_t Kt, const int32_t *labels_true, int64_t *table_out)
{
    GEMHIP_REQUIRE(h != nullptr, "kmeans_contingency: NULL handle");
    GEMHIP_REQUIRE(h->have_labels, "kmeans_contingency: no labels on the device (gemhip_kmeans_fit, _assign or _update first)");
    GEMHIP_REQUIRE(Kt >= 1, "kmeans_contingency: Kt = %d (need >= 1)", Kt);
    GEMHIP_REQUIRE(labels_true && table_out, "kmeans_contingency: NULL argument");
    if ((int64_t)h->K * Kt > KM_MAX_TABLE) return fail(GEMHIP_E_UNSUPPORTED, "kmeans_contingency: a %d x %d table: at most 2^26 entries", h->K, Kt);
    const int64_t bad = first_bad_index(labels_true, h->n, Kt);
    GEMHIP_REQUIRE(bad < 0, "kmeans_contingency: true label %lld = %d outside [0,%d)", (long long)bad, labels_true[bad], Kt);
    const size_t cells = (size_t)h->K * Kt;
    GEMHIP_CHECK(h->true_lab.upload(labels_true, (size_t)h->n));
    GEMHIP_CHECK(h->table.reserve(cells));
    GEMHIP_CHECK(hipMemsetAsync(h->table, 0, cells * sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(km_contingency_kernel, dim3(grid_of(h->n, 256)), dim3(256), 0, 0, h->labels.get(), h->true_lab.get(), h->n, Kt, h->table.get());
    GEMHIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> t(cells);
    GEMHIP_CHECK(hipMemcpy(t.data(), h->table, cells * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < cells; ++q) table_out[q] = (int64_t)t[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_clustering_scores_host(const int64_t *table, int32_t Kp, int32_t Kt, double *out)
{
    GEMHIP_REQUIRE(table && out, "clustering_scores_host: NULL argument");
    GEMHIP_REQUIRE(Kp >= 1 && Kt >= 1, "clustering_scores_host: a %d x %d table (need at least 1 x 1)", Kp, Kt);
    for (size_t q = 0; q < (size_t)Kp * Kt; ++q)
        GEMHIP_REQUIRE(table[q] >= 0, "clustering_scores_host: table[%lld][%lld] = %lld is negative", (long long)(q / Kt), (long long)(q % Kt), (long long)table[q]);
    GEMHIP_REQUIRE(km_scores(table, Kp, Kt, out), "clustering_scores_host: the table is empty");
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_last_ms(gemhip_kmeans_t h, double *out)
{
    GEMHIP_REQUIRE(h && out, "kmeans_last_ms: NULL");
    for (int q = 0; q < 6; ++q) out[q] = h->ms[q];
    return GEMHIP_OK;
}

extern "C" int gemhip_kmeans_info(gemhip_kmeans_t h, int64_t *out)
{
    GEMHIP_REQUIRE(h && out, "kmeans_info: NULL");
    out[0] = h->n; out[1] = h->d; out[2] = h->dpad; out[3] = h->have_labels ? h->K : 0; out[4] = KM_ROWS; out[5] = KM_CT; out[6] = KM_MAX_D; out[7] = KM_MAX_K;
    out[8] = KM_MAX_TRIALS; out[9] = KM_SLICE; out[10] = h->slab_rows; out[11] = h->iterations;
    return GEMHIP_OK;
}
