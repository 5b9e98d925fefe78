// eval_common.hpp -- what the evaluation units (eval, rank, tsne, nc, kmeans, edgeclf, nbr .hip) share on the HIP side: the grid size of a
// launch, the host wall clock and the event stopwatch behind their ms[] slots, the wording of the refusals every unit makes of an embedding
// matrix, and the fixed-shape fp64 sum.  The device-free half of the ingest (the scans that find what to refuse) is matrix_host.hpp.
#pragma once
#include "common.hpp"
#include "matrix_host.hpp"
#include <chrono>
#include <climits>

namespace gemhip {

// Workgroups of `per` items that cover `count` items, at least one.  A capped grid is min(grid_of(...), cap).
inline unsigned grid_of(int64_t count, int64_t per) { return (unsigned)((count + per - 1) / per < 1 ? 1 : (count + per - 1) / per); }

// Host wall clock, milliseconds: the ms[] slots documented as wall time in include/gem_hip.h.
inline double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Device time between two marks on the null stream: the ms[] slots documented as event time.  The events are made on first use.
using Stopwatch = EventMarks<2>;
inline hipError_t start(Stopwatch &w) { const hipError_t e = w.create(); return e != hipSuccess ? e : w.mark(0); }
inline hipError_t stop(Stopwatch &w, double *ms) { const hipError_t e = w.mark(1); return e != hipSuccess ? e : w.ms(0, 1, ms); }      // waits for the stream

// The refusals every unit makes of an embedding matrix X [n][ld] with d live columns, in this order: n below min_n, d outside [1, ld],
// n not below 2^31, d above max_d (max_d_reason says what the limit comes from; max_d = 0: the unit has none), X == NULL.  The scan of the
// entries is first_bad_entry (matrix_host.hpp); its refusal is the unit's own.
inline int check_embedding(const char *who, int64_t n, int32_t d, int64_t ld, const float *X, int min_n, int max_d, const char *max_d_reason)
{
    GEMHIP_REQUIRE(n >= min_n, "%s: n = %lld (need n >= %d)", who, (long long)n, min_n);
    GEMHIP_REQUIRE(d >= 1 && ld >= d, "%s: d = %d, ld = %lld (need 1 <= d <= ld)", who, d, (long long)ld);
    if (n > INT32_MAX) return fail(GEMHIP_E_UNSUPPORTED, "%s: n = %lld: must be below 2^31", who, (long long)n);
    if (max_d && d > max_d) return fail(GEMHIP_E_UNSUPPORTED, "%s: d = %d: at most %d (%s)", who, d, max_d, max_d_reason);
    GEMHIP_REQUIRE(X != nullptr, "%s: NULL X", who);
    return GEMHIP_OK;
}

#if defined(__HIPCC__)
// *out = sum of v[0 .. n): ONE workgroup of BLOCK threads; a thread's elements in index order, then a fixed tree.  Owner is the handle type
// of the unit that launches it: one instantiation per unit, so that no kernel symbol is defined in two units of the library.
template <int BLOCK, typename Owner>
__global__ __launch_bounds__(BLOCK) void block_sum_f64_kernel(const double *__restrict__ v, int64_t n, double *__restrict__ out)
{
    __shared__ double s[BLOCK];
    double a = 0.0;
    for (int64_t t = threadIdx.x; t < n; t += BLOCK) a += v[t];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int off = BLOCK / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s[threadIdx.x] += s[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}
#endif

}  // namespace gemhip
