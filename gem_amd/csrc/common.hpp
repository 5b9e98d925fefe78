// common.hpp -- shared host/device helpers for libgem_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <cstdio>
#include <cstdarg>

#include "../../include/gem_hip.h"

namespace gemhip {

// ---------------------------------------------------------------- error state
std::string &last_error_ref();
int fail(int code, const char *fmt, ...);

#define GEMHIP_CHECK(expr)                                                        \
    do {                                                                          \
        hipError_t _e = (expr);                                                   \
        if (_e != hipSuccess)                                                     \
            return ::gemhip::fail(GEMHIP_E_HIP, "%s failed: %s (%s:%d)", #expr,   \
                                  hipGetErrorString(_e), __FILE__, __LINE__);     \
    } while (0)

#define GEMHIP_REQUIRE(cond, ...)                                  \
    do {                                                           \
        if (!(cond))                                               \
            return ::gemhip::fail(GEMHIP_E_INVALID, __VA_ARGS__);  \
    } while (0)

// ---------------------------------------------------------------- where a one-shot call's wall time went (gemhip_last_call_phases)
// Thread-local accumulators the one-shot entry points (gemhip_gf_train, gemhip_n2v_train, gemhip_hope) reset on entry; the staged calls they
// are made of add host-side preparation (sorting, Vose tables), host->device and device->host copy time to them.  Wall-clock, host side.
enum { PH_TOTAL = 0, PH_HOST = 1, PH_H2D = 2, PH_KERNELS = 3, PH_D2H = 4, PH_COUNT = 8 };
double *phase_acc();
double phase_now();
struct PhaseScope {
    int k; double t0;
    explicit PhaseScope(int kk) : k(kk), t0(phase_now()) {}
    ~PhaseScope() { phase_acc()[k] += phase_now() - t0; }
};

// ---------------------------------------------------------------- owned memory
// The one owner of device (DevBuf) and pinned host (PinnedBuf) memory in this library: move-only, frees in its destructor on the device it
// allocated on.  Converts to T* for kernel arguments and copies.  Memory the library only borrows from a caller stays a plain T* view.
template <typename T, bool PINNED>
class Buf {
    T *p_ = nullptr; size_t cap_ = 0; int dev_ = 0;
    void release(bool wait)       // free on the block's own device, then back to the caller's (if the current device cannot be read: on whichever is current)
    {
        if (!p_) return;
        int cur = dev_;
        const bool hop = hipGetDevice(&cur) == hipSuccess && cur != dev_;
        if (hop) (void)hipSetDevice(dev_);
        if (wait) (void)hipDeviceSynchronize();          // (a failure here is not lost: the free below synchronises too, and the next call reports it)
        (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
        if (hop) (void)hipSetDevice(cur);
        p_ = nullptr; cap_ = 0;
    }
public:
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p_(o.p_), cap_(o.cap_), dev_(o.dev_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; dev_ = o.dev_; o.p_ = nullptr; o.cap_ = 0; } return *this; }
    ~Buf() { reset(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }          // elements asked for by the reserve() that allocated the block
    void reset() { release(false); }
    // Grow-only, contents NOT preserved.  Holding a block of >= count elements: no HIP call at all.  Otherwise: wait for the block's device (a launch
    // in flight may still read the old block), free it, allocate at least 16 bytes on the current device (so an empty buffer's reserve(0) still
    // yields a valid pointer: empty graphs).  On failure the buffer is empty.
    hipError_t reserve(size_t count)
    {
        if (p_ && count <= cap_) return hipSuccess;
        release(true);
        const size_t bytes = count * sizeof(T) > 16 ? count * sizeof(T) : 16;
        hipError_t e = hipGetDevice(&dev_);
        if (e == hipSuccess) e = PINNED ? hipHostMalloc((void **)&p_, bytes, hipHostMallocDefault) : hipMalloc((void **)&p_, bytes);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        cap_ = count;
        return hipSuccess;
    }
    hipError_t upload(const T *host, size_t count)     // reserve + blocking copy from pageable or pinned host memory
    {
        const hipError_t e = reserve(count);
        return e != hipSuccess || !count ? e : hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice);
    }
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using PinnedBuf = Buf<T, true>;

// ---------------------------------------------------------------- owned timing events
// The one owner of the library's timing events: N marks, move-only, destroyed in the destructor.  (Ordering events made with
// hipEventDisableTiming -- GF's hub fork/join, HOPE's CoefSlot::done -- and HOPE's growing SpMM pool are not marks and stay where they are.)
template <int N>
struct EventMarks {
    hipEvent_t ev[N] = {};
    EventMarks() = default;
    EventMarks(const EventMarks &) = delete;
    EventMarks &operator=(const EventMarks &) = delete;
    EventMarks(EventMarks &&o) noexcept { take(o); }
    EventMarks &operator=(EventMarks &&o) noexcept { if (this != &o) { destroy(); take(o); } return *this; }
    ~EventMarks() { destroy(); }
    hipError_t create()                                             // idempotent: makes the events that are not there yet
    {
        for (hipEvent_t &e : ev) if (!e) { const hipError_t r = hipEventCreate(&e); if (r != hipSuccess) { e = nullptr; return r; } }
        return hipSuccess;
    }
    hipError_t mark(int k, hipStream_t s = 0) { return hipEventRecord(ev[k], s); }
    hipError_t ms(int from, int to, double *out)                    // waits for mark `to`; *out is written on success only
    {
        hipError_t e = hipEventSynchronize(ev[to]);
        float f = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&f, ev[from], ev[to]);
        if (e == hipSuccess) *out = f;
        return e;
    }
private:
    void destroy() { for (hipEvent_t &e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
    void take(EventMarks &o) { for (int k = 0; k < N; ++k) { ev[k] = o.ev[k]; o.ev[k] = nullptr; } }
};

constexpr int WAVE = 64;          // CDNA wavefront
constexpr int NUM_XCD = 8;        // MI355X: 8 XCDs, block b lands on XCD b % 8

// ---------------------------------------------------------------- device side
#if defined(__HIPCC__)

// Wave-wide fp32 sum, result in every lane.  4 DPP steps reduce inside each
// row of 16 lanes (no LDS traffic), then 4 v_readlane fold the four rows.
__device__ __forceinline__ float wave_sum(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));  // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)); // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)); // row_mirror
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}

// Wave-wide fp64 sum by a butterfly: the same bits in every lane.
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }

template <typename T>
__device__ __forceinline__ T bcast_lane(T v, int srclane)   // srclane must be wave-uniform
{
    static_assert(sizeof(T) == 4, "32-bit only");
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), srclane));
}

// XCD-aware work mapping: hardware places block b on XCD b % 8.  Give every XCD
// one CONTIGUOUS eighth of the work-item range so that neighbouring rows (which
// share most of their gather targets in block-structured graphs) meet in the
// same 4 MiB L2.  Speed only -- correctness never depends on placement.
__device__ __forceinline__ int64_t xcd_contiguous_block(int64_t b, int64_t nblocks)
{
    const int64_t per = (nblocks + NUM_XCD - 1) / NUM_XCD;
    const int64_t xcd = b % NUM_XCD, idx = b / NUM_XCD;
    return xcd * per + idx;        // may be >= nblocks for the ragged tail: caller checks
}

// ------------------------------------------------------------- Philox4x32-10
// Counter-based RNG (Salmon et al. 2011).  Stateless: every draw is a pure
// function of (seed, counter), so the CPU oracle reproduces the device stream
// exactly and results do not depend on scheduling.
struct u32x4 { uint32_t x, y, z, w; };

__host__ __device__ __forceinline__ u32x4 philox4x32_10(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3)
{
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

// uniform in [0,1) with 24 bits, exactly representable in fp32
__host__ __device__ __forceinline__ float u01(uint32_t r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }

#endif  // __HIPCC__

}  // namespace gemhip
