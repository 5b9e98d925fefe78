// multi.hip -- the N-GPU entry points of the C ABI: ONE process drives n_gpus devices, collectives over RCCL (xGMI).
//
// the reference has no multi-device path (`grep -r nccl\|mpi /root/reference` is empty); north_star shards GF by source row and
// node2vec by start node.  A GEM maintainer who binds libgem_hip.so gets that from two calls that mirror the one-shot drop-ins and take n_gpus:
//   gemhip_gf_train_multi    gf.py:81-101 / `gf <graph> <emb> ...` -- source rows in N contiguous blocks, the table replicated, an in-place
//                            ncclAllGather of the owned row blocks after EVERY sweep: bit-identical to gemhip_gf_train (exchange after every
//                            sweep is what keeps gf.py:93-100's Gauss-Seidel order across ranks)
//   gemhip_n2v_train_multi   node2vec.py:27-54 -- walks by start-node shard, ncclAllReduce of the token counts, ONE ncclAllGather of the walk
//                            shards, then the partitioned-table schedule: rank g keeps SynPos partition g, trains the bucket
//                            (g, (g+s) % N) of each episode in walk order (gemhip_sgns_train_part) and passes its SynNeg partition around a ring
//                            (ncclSend / ncclRecv) between rounds
// gem_amd/multi_gpu.py drives the same schedules with one process per GPU over torch.distributed (what bench.py --gpus N launches); this file is the
// same thing for a host that is not Python.  RCCL is loaded with dlopen on first use (librccl.so.1), so the library itself has no link-time
// dependency on it and every single-GPU entry point works on a box without RCCL.
//
// Test mode: a device list with REPEATED entries (e.g. {0, 0, 0, 0}) runs the ranks as VIRTUAL ranks on one device -- RCCL refuses two ranks on one
// GPU, so the three collectives are then plain device-to-device copies on one stream; everything else (sharding, episode table, bucket order, ring)
// is the production code.  That is how the one-GPU test box checks N > 1 (tests/test_multi_capi_gpu.py).
//
// What the two drivers compute before and between their device steps -- shards, row blocks, the edge orders GF can shard, the episode table, alpha's
// token offsets, the cut and paste of a table partition -- is host arithmetic in multi_plan.hip (no HIP; tests/test_multi_plan.py holds it against
// gem_amd/multi_gpu.py on the CPU).  This file words the refusals and issues the device steps over such a plan.
#include "common.hpp"
#include "multi_plan.hpp"
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <vector>
#include <string>
#include <algorithm>
#include <cstring>
#include <chrono>

using namespace gemhip;

namespace {

struct RcclApi {
    void *lib = nullptr;
    std::string why;                         // dlerror() text of the failed dlopen / the first missing symbol (dlerror clears itself when read)
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool ok = false;
};

RcclApi &rccl()
{
    static RcclApi R;
    if (R.lib || R.ok) return R;
    // The RCCL that belongs to the HIP runtime THIS library is bound to: a process can hold two (PyTorch ships its own libamdhip64 / libhsa-runtime64 /
    // librccl next to /opt/rocm's), and an RCCL bound to the other, never-initialised runtime fails inside ncclCommInitAll with "no ROCm-capable device"
    // (seen in round 6 when torch was imported AFTER this library: dlopen("librccl.so.1") then returned torch's copy by soname).  dladdr on a HIP entry
    // point names the runtime in use; its directory is searched first.
    std::vector<std::string> names;
    {
        Dl_info info;
        if (dladdr((void *)&hipGetDeviceCount, &info) && info.dli_fname) {
            std::string dir(info.dli_fname);
            const size_t cut = dir.rfind('/');
            if (cut != std::string::npos) { dir.resize(cut); names.push_back(dir + "/librccl.so.1"); names.push_back(dir + "/librccl.so"); }
        }
    }
    for (const char *fallback : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) names.push_back(fallback);
    for (const std::string &name : names) {
        R.lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (R.lib) break;
        const char *e = dlerror();
        if (R.why.empty() && e) R.why = e;
    }
    if (!R.lib) return R;
    R.why.clear();
#define GEMHIP_RCCL_SYM(f)                                                                             \
    do {                                                                                               \
        R.f = (decltype(R.f))dlsym(R.lib, "nccl" #f);                                                  \
        if (!R.f && R.why.empty()) R.why = "symbol nccl" #f " missing";                                \
    } while (0)
    GEMHIP_RCCL_SYM(CommInitAll); GEMHIP_RCCL_SYM(CommDestroy); GEMHIP_RCCL_SYM(AllGather); GEMHIP_RCCL_SYM(AllReduce); GEMHIP_RCCL_SYM(Send);
    GEMHIP_RCCL_SYM(Recv); GEMHIP_RCCL_SYM(GroupStart); GEMHIP_RCCL_SYM(GroupEnd); GEMHIP_RCCL_SYM(GetErrorString);
#undef GEMHIP_RCCL_SYM
    R.ok = R.CommInitAll && R.CommDestroy && R.AllGather && R.AllReduce && R.Send && R.Recv && R.GroupStart && R.GroupEnd && R.GetErrorString;
    return R;
}

#define NCCL_TRY(x)                                                                                                     \
    do {                                                                                                                \
        ncclResult_t _r = (x);                                                                                          \
        if (_r != ncclSuccess) return fail(GEMHIP_E_HIP, "%s failed: %s (%s:%d)", #x, rccl().GetErrorString(_r), __FILE__, __LINE__); \
    } while (0)

// inside an open ncclGroupStart: the group is closed before the error is returned (a dangling group would swallow every later call of the thread)
#define NCCL_TRY_IN_GROUP(x)                                                                                            \
    do {                                                                                                                \
        ncclResult_t _r = (x);                                                                                          \
        if (_r != ncclSuccess) {                                                                                        \
            rccl().GroupEnd();                                                                                          \
            return fail(GEMHIP_E_HIP, "%s failed: %s (%s:%d)", #x, rccl().GetErrorString(_r), __FILE__, __LINE__);      \
        }                                                                                                               \
    } while (0)

__global__ void add_i32_kernel(int32_t *__restrict__ acc, const int32_t *__restrict__ x, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[i] += x[i];
}

// a step of an entry point that returns the library's own code
#define GEMHIP_TRY(x) do { if (int _rc = (x)) return _rc; } while (0)

// The ranks of one call: devices, one stream per rank, and the three collectives the schedules need.  Owns the communicators and the streams.  An
// entry point declares its device buffers BEFORE the fabric and its per-rank handles AFTER it, so that on every way out the handles go first, then
// the communicators, then every stream is drained and destroyed on its own device and the caller's device restored, and only then the buffers are freed.
struct Fabric {
    int N = 0;
    bool virt = false;                       // repeated devices: virtual ranks on one stream, copies instead of RCCL
    bool always_rccl = false;                // also route the (trivial) 1-rank collectives through RCCL (gemhip_rccl_selftest)
    std::vector<int> dev;
    std::vector<hipStream_t> st;
    std::vector<ncclComm_t> comm;
    int prev_dev = 0;

    Fabric() = default;
    Fabric(const Fabric &) = delete;
    Fabric &operator=(const Fabric &) = delete;
    ~Fabric()
    {
        for (int r = 0; r < (int)comm.size(); ++r) if (comm[r]) rccl().CommDestroy(comm[r]);
        for (int r = 0; r < (virt ? std::min(N, 1) : N); ++r)
            if (r < (int)st.size() && st[r]) { (void)hipSetDevice(dev[r]); (void)hipStreamSynchronize(st[r]); (void)hipStreamDestroy(st[r]); }
        (void)hipSetDevice(prev_dev);
    }

    int init(int32_t n_gpus, const int32_t *devices)
    {
        GEMHIP_REQUIRE(n_gpus >= 1 && n_gpus <= 64, "n_gpus=%d (1..64)", n_gpus);
        int count = 0;
        GEMHIP_CHECK(hipGetDeviceCount(&count));
        GEMHIP_CHECK(hipGetDevice(&prev_dev));
        N = n_gpus;
        dev.resize(N);
        for (int r = 0; r < N; ++r) {
            dev[r] = devices ? devices[r] : r;
            GEMHIP_REQUIRE(dev[r] >= 0 && dev[r] < count, "rank %d: device %d of %d visible (pass a device list with repeats to run VIRTUAL ranks on one GPU)", r, dev[r], count);
        }
        std::vector<int> u(dev); std::sort(u.begin(), u.end());
        virt = std::adjacent_find(u.begin(), u.end()) != u.end();
        if (virt) GEMHIP_REQUIRE(u.front() == u.back(), "virtual ranks: all ranks must name the SAME device");
        st.assign(N, nullptr);
        if (virt) {
            GEMHIP_CHECK(hipSetDevice(dev[0]));
            hipStream_t s = nullptr;
            GEMHIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            for (int r = 0; r < N; ++r) st[r] = s;
            return GEMHIP_OK;
        }
        for (int r = 0; r < N; ++r) {
            GEMHIP_CHECK(hipSetDevice(dev[r]));
            GEMHIP_CHECK(hipStreamCreateWithFlags(&st[r], hipStreamNonBlocking));
        }
        RcclApi &R = rccl();
        if (!R.ok) return fail(GEMHIP_E_UNSUPPORTED, "librccl.so.1 could not be loaded (%s): the multi-GPU entry points need RCCL", R.why.empty() ? "unknown reason" : R.why.c_str());
        comm.assign(N, nullptr);
        (void)hipGetLastError();         // a sticky error left by an earlier, unrelated launch of this process would surface inside RCCL's init as "unhandled cuda error"
        NCCL_TRY(R.CommInitAll(comm.data(), N, dev.data()));
        return GEMHIP_OK;
    }
    int use(int r) { GEMHIP_CHECK(hipSetDevice(dev[r])); return GEMHIP_OK; }
    int sync_all()
    {
        // the DEVICE, not only the rank's stream: the streams are non-blocking, i.e. not ordered with the null stream, which the library calls between
        // the phases use for their own set-up (gemhip_sgns_init, the unigram builders, the blocking uploads).  The drivers' own device-side copies and
        // memsets are issued on st[r], so their order with the kernels does not rest on this wait.
        for (int r = 0; r < (virt ? 1 : N); ++r) { GEMHIP_CHECK(hipSetDevice(dev[r])); GEMHIP_CHECK(hipStreamSynchronize(st[r])); GEMHIP_CHECK(hipDeviceSynchronize()); }
        return GEMHIP_OK;
    }
    // every rank's buf holds N blocks of `bytes`; block r of rank r is valid on entry, all blocks on every rank on exit
    int all_gather_inplace(const std::vector<void *> &buf, size_t bytes)
    {
        if (N == 1 && !always_rccl) return GEMHIP_OK;
        if (virt) {
            for (int r = 0; r < N; ++r)
                for (int q = 0; q < N; ++q)
                    if (q != r) GEMHIP_CHECK(hipMemcpyAsync((char *)buf[q] + (size_t)r * bytes, (const char *)buf[r] + (size_t)r * bytes, bytes, hipMemcpyDeviceToDevice, st[0]));
            return GEMHIP_OK;
        }
        RcclApi &R = rccl();
        NCCL_TRY(R.GroupStart());
        for (int r = 0; r < N; ++r) NCCL_TRY_IN_GROUP(R.AllGather((const char *)buf[r] + (size_t)r * bytes, buf[r], bytes, ncclInt8, comm[r], st[r]));
        NCCL_TRY(R.GroupEnd());
        return GEMHIP_OK;
    }
    int all_reduce_sum_i32(const std::vector<int32_t *> &buf, int64_t count)
    {
        if (N == 1 && !always_rccl) return GEMHIP_OK;
        if (virt) {
            for (int r = 1; r < N; ++r) hipLaunchKernelGGL(add_i32_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st[0], buf[0], buf[r], count);
            for (int r = 1; r < N; ++r) GEMHIP_CHECK(hipMemcpyAsync(buf[r], buf[0], (size_t)count * 4, hipMemcpyDeviceToDevice, st[0]));
            GEMHIP_CHECK(hipGetLastError());
            return GEMHIP_OK;
        }
        RcclApi &R = rccl();
        NCCL_TRY(R.GroupStart());
        for (int r = 0; r < N; ++r) NCCL_TRY_IN_GROUP(R.AllReduce(buf[r], buf[r], (size_t)count, ncclInt32, ncclSum, comm[r], st[r]));
        NCCL_TRY(R.GroupEnd());
        return GEMHIP_OK;
    }
    // rank r sends `send[r]` to rank r-1 and receives rank r+1's into `recv[r]`
    int ring_shift(const std::vector<void *> &send, const std::vector<void *> &recv, size_t bytes)
    {
        if (N == 1 && !always_rccl) { if (send[0] != recv[0]) GEMHIP_CHECK(hipMemcpyAsync(recv[0], send[0], bytes, hipMemcpyDeviceToDevice, st[0])); return GEMHIP_OK; }
        if (virt) {
            for (int r = 0; r < N; ++r) GEMHIP_CHECK(hipMemcpyAsync(recv[r], send[(r + 1) % N], bytes, hipMemcpyDeviceToDevice, st[0]));
            return GEMHIP_OK;
        }
        RcclApi &R = rccl();
        NCCL_TRY(R.GroupStart());
        for (int r = 0; r < N; ++r) {
            NCCL_TRY_IN_GROUP(R.Send(send[r], bytes, ncclInt8, (r + N - 1) % N, comm[r], st[r]));
            NCCL_TRY_IN_GROUP(R.Recv(recv[r], bytes, ncclInt8, (r + 1) % N, comm[r], st[r]));
        }
        NCCL_TRY(R.GroupEnd());
        return GEMHIP_OK;
    }
};

// One rank's library handle (a GF plan, a node2vec handle): move-only, released on the rank's device.
template <typename H, int (*DESTROY)(H)>
struct RankHandle {
    H h = nullptr;
    int dev = 0;
    RankHandle() = default;
    RankHandle(RankHandle &&o) noexcept : h(o.h), dev(o.dev) { o.h = nullptr; }
    RankHandle &operator=(RankHandle &&o) noexcept { std::swap(h, o.h); std::swap(dev, o.dev); return *this; }
    ~RankHandle() { if (h) { (void)hipSetDevice(dev); DESTROY(h); } }
};
using RankGfPlan = RankHandle<gemhip_gf_plan_t, gemhip_gf_plan_destroy>;
using RankN2v = RankHandle<gemhip_n2v_t, gemhip_n2v_destroy>;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

using Bytes = DevBuf<char>;
int alloc_on(Bytes &b, int device, size_t bytes) { GEMHIP_CHECK(hipSetDevice(device)); GEMHIP_CHECK(b.reserve(bytes)); return GEMHIP_OK; }

}  // namespace

// Communicator round trip: create over n_gpus devices, run the three collectives of the schedules on known patterns (`bytes` per rank), verify every
// byte, destroy.  The GPU tier runs it with n_gpus = 1 (RCCL itself: a 1-rank all-gather is a copy) and with virtual ranks.
extern "C" int gemhip_rccl_selftest(int32_t n_gpus, const int32_t *devices, int64_t bytes, double *seconds)
{
    GEMHIP_REQUIRE(bytes >= 4 && bytes % 4 == 0 && bytes <= ((int64_t)1 << 30), "rccl_selftest: bytes=%lld (multiple of 4, <= 1 GiB)", (long long)bytes);
    GEMHIP_REQUIRE(n_gpus >= 1 && n_gpus <= 64, "rccl_selftest: n_gpus=%d (1..64)", n_gpus);
    const int N = n_gpus;
    const int64_t words = bytes / 4;
    std::vector<Bytes> G(N), A(N), S(N), Rv(N);
    Fabric F;
    F.always_rccl = true;                    // n_gpus = 1 exercises RCCL itself: a 1-rank all-gather / all-reduce / self send-recv
    GEMHIP_TRY(F.init(n_gpus, devices));
    std::vector<void *> g(N), s(N), rv(N);
    std::vector<int32_t *> a(N);
    const double t0 = now_s();
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(alloc_on(G[r], F.dev[r], (size_t)bytes * N));
        GEMHIP_TRY(alloc_on(A[r], F.dev[r], (size_t)bytes));
        GEMHIP_TRY(alloc_on(S[r], F.dev[r], (size_t)bytes));
        GEMHIP_TRY(alloc_on(Rv[r], F.dev[r], (size_t)bytes));
        g[r] = G[r].get(); a[r] = (int32_t *)A[r].get(); s[r] = S[r].get(); rv[r] = Rv[r].get();
        std::vector<int32_t> h((size_t)words * N, -1), hb((size_t)words);
        for (int64_t i = 0; i < words; ++i) { h[(size_t)r * words + i] = (int32_t)(1000003 * r + i); hb[i] = (int32_t)((r + 1) * (i % 97 + 1)); }
        if (hipMemcpy(g[r], h.data(), (size_t)bytes * N, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(a[r], hb.data(), bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(s[r], hb.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
            return fail(GEMHIP_E_HIP, "rccl_selftest: upload failed");
    }
    GEMHIP_TRY(F.all_gather_inplace(g, (size_t)bytes));
    GEMHIP_TRY(F.all_reduce_sum_i32(a, words));
    GEMHIP_TRY(F.ring_shift(s, rv, (size_t)bytes));
    GEMHIP_TRY(F.sync_all());
    for (int r = 0; r < N; ++r) {
        std::vector<int32_t> h((size_t)words * N), ha((size_t)words), hr((size_t)words);
        GEMHIP_TRY(F.use(r));
        if (hipMemcpy(h.data(), g[r], (size_t)bytes * N, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(ha.data(), a[r], bytes, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hr.data(), rv[r], bytes, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(GEMHIP_E_HIP, "rccl_selftest: download failed");
        for (int q = 0; q < N; ++q)
            for (int64_t i = 0; i < words; ++i)
                if (h[(size_t)q * words + i] != (int32_t)(1000003 * q + i)) return fail(GEMHIP_E_HIP, "rccl_selftest: all-gather: rank %d block %d word %lld wrong", r, q, (long long)i);
        const int64_t tri = (int64_t)N * (N + 1) / 2;
        for (int64_t i = 0; i < words; ++i) {
            if (ha[i] != (int32_t)(tri * (i % 97 + 1))) return fail(GEMHIP_E_HIP, "rccl_selftest: all-reduce: rank %d word %lld wrong", r, (long long)i);
            if (hr[i] != (int32_t)(((r + 1) % N + 1) * (i % 97 + 1))) return fail(GEMHIP_E_HIP, "rccl_selftest: ring shift: rank %d word %lld wrong", r, (long long)i);
        }
    }
    if (seconds) *seconds = now_s() - t0;
    return GEMHIP_OK;
}

// gf.py:81-101 on n_gpus devices.  stats (optional, 8 doubles): {seconds of the sweeps incl. exchanges (wall, all ranks synchronised), updates per
// sweep (all ranks), rows per sweep, exchange bytes per rank per sweep, n_gpus, virtual ranks (0/1), 0, 0}.
extern "C" int gemhip_gf_train_multi(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int32_t d, float eta, float regu,
                                     int32_t max_iter, int32_t n_gpus, const int32_t *devices, float *X_inout, double *stats)
{
    GEMHIP_REQUIRE(X_inout != nullptr && max_iter >= 0 && n > 0 && m >= 0 && d >= 1, "gf_train_multi: bad arguments");
    GEMHIP_REQUIRE(n_gpus >= 1 && n_gpus <= 64, "gf_train_multi: n_gpus=%d (1..64)", n_gpus);          // before anything is sized or divided by it
    if (n_gpus > 1) {                        // other edge orders need one GPU (the rule: multi_plan.hpp)
        const GfShardError e = gf_check_shardable(n, m, src, dst);
        GEMHIP_REQUIRE(e.kind != GfShardError::EDGE_OUT_OF_RANGE, "gf_train_multi: edge %lld out of range", (long long)e.edge);
        if (e) return fail(GEMHIP_E_UNSUPPORTED, "gf_train_multi: firing sources are not first visited in ascending id order (row %d after row %lld): "
                                                 "sharding by source row would change the reference's Gauss-Seidel order; use n_gpus = 1", (int)e.row, (long long)e.after);
    }
    const int N = n_gpus;
    const GfRowBlocks B = gf_row_blocks(n, N);
    const size_t table_bytes = (size_t)B.n_pad * d * sizeof(float), block_bytes = (size_t)B.block * d * sizeof(float);
    std::vector<Bytes> Xa(N), Xb(N);
    Fabric F;
    GEMHIP_TRY(F.init(n_gpus, devices));
    std::vector<RankGfPlan> plan(N);
    std::vector<float> Xpad;
    if (B.n_pad != n) { Xpad.assign((size_t)B.n_pad * d, 0.f); std::memcpy(Xpad.data(), X_inout, (size_t)n * d * sizeof(float)); }
    const float *Xsrc = B.n_pad != n ? Xpad.data() : X_inout;
    double upd = 0, rows = 0;
    for (int r = 0; r < N; ++r) {
        const Range own = B.rows(r);
        GEMHIP_TRY(F.use(r));
        plan[r].dev = F.dev[r];
        GEMHIP_TRY(gemhip_gf_plan_create(n, m, src, dst, w, d, own.lo, own.hi, &plan[r].h));
        GEMHIP_TRY(alloc_on(Xa[r], F.dev[r], table_bytes));
        GEMHIP_TRY(alloc_on(Xb[r], F.dev[r], table_bytes));
        // the upload is complete when it returns (pageable host memory); the copy Xb <- Xa is ordered with the sweeps by the rank's stream
        if (hipMemcpy(Xa[r].get(), Xsrc, table_bytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpyAsync(Xb[r].get(), Xa[r].get(), table_bytes, hipMemcpyDeviceToDevice, F.st[r]) != hipSuccess)
            return fail(GEMHIP_E_HIP, "gf_train_multi: table upload failed on rank %d", r);
        GEMHIP_TRY(gemhip_gf_plan_bind(plan[r].h, Xa[r].get(), Xb[r].get()));
        int64_t info[8];
        GEMHIP_TRY(gemhip_gf_plan_info(plan[r].h, info));
        upd += (double)info[0]; rows += (double)info[1];
    }
    GEMHIP_TRY(F.sync_all());
    const double t0 = now_s();
    std::vector<void *> cur(N);
    for (int it = 0; it < max_iter; ++it) {
        for (int r = 0; r < N; ++r) {
            GEMHIP_TRY(F.use(r));
            GEMHIP_TRY(gemhip_gf_plan_sweeps(plan[r].h, 1, eta, regu, F.st[r]));
            GEMHIP_TRY(gemhip_gf_plan_current(plan[r].h, &cur[r]));
        }
        GEMHIP_TRY(F.all_gather_inplace(cur, block_bytes));          // owned row blocks -> every rank holds the whole new table
    }
    GEMHIP_TRY(F.sync_all());
    const double el = now_s() - t0;
    void *p0 = nullptr;
    GEMHIP_TRY(F.use(0));
    GEMHIP_TRY(gemhip_gf_plan_current(plan[0].h, &p0));
    if (hipMemcpy(X_inout, p0, (size_t)n * d * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return fail(GEMHIP_E_HIP, "gf_train_multi: download failed");
    if (stats) {
        stats[0] = el; stats[1] = upd; stats[2] = rows; stats[3] = N > 1 ? (double)(N - 1) * B.block * d * 4.0 : 0.0; stats[4] = N; stats[5] = F.virt ? 1.0 : 0.0;
        stats[6] = 0.0; stats[7] = 0.0;
    }
    return GEMHIP_OK;
}

// node2vec.py:27-54 on n_gpus devices (module comment).  `episodes` slices of every rank's walk shard (64 = the default of gem_amd/multi_gpu.py; the
// SynNeg partitions complete one ring tour per episode).  stats (optional, 8 doubles): {walk + vocabulary + gather seconds, training seconds (wall, all
// ranks synchronised), tokens, pairs trained (all ranks), ring-shift bytes per rank per round, n_gpus, virtual ranks (0/1), bucket launches per rank}.
extern "C" int gemhip_n2v_train_multi(int64_t n, int64_t nnz, const int64_t *row_ptr, const int32_t *col, const float *w, int32_t d, int32_t walk_len,
                                      int32_t num_walks, int32_t window, int32_t epochs, float p, float q, uint64_t seed, int32_t flags, int32_t n_gpus,
                                      const int32_t *devices, int32_t episodes, float *X_out, double *stats)
{
    GEMHIP_REQUIRE(X_out != nullptr && episodes >= 1 && epochs >= 1 && epochs < 256, "n2v_train_multi: bad arguments (episodes=%d epochs=%d)", episodes, epochs);
    GEMHIP_REQUIRE(n_gpus >= 1 && n_gpus <= 64, "n2v_train_multi: n_gpus=%d (1..64)", n_gpus);         // before anything is sized or divided by it
    const int N = n_gpus;
    std::vector<Bytes> corpus(N), segd(N), Pp(N), Na(N), Nb(N);
    Fabric F;
    GEMHIP_TRY(F.init(n_gpus, devices));
    std::vector<RankN2v> h(N);
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(F.use(r));
        h[r].dev = F.dev[r];
        GEMHIP_TRY(gemhip_n2v_create(n, nnz, row_ptr, col, w, &h[r].h));
    }
    int64_t m_start = 0;
    GEMHIP_TRY(gemhip_n2v_start_nodes(h[0].h, &m_start));
    const int64_t total = m_start * (int64_t)num_walks;
    const N2vMultiPlan P = n2v_multi_plan(total, N, episodes, walk_len, n, epochs);
    const double t0 = now_s();
    // ---- walks of my start-node shard, token counts summed over the ranks
    std::vector<int32_t *> cnt(N, nullptr);
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(F.use(r));
        GEMHIP_TRY(gemhip_n2v_walks(h[r].h, p, q, num_walks, walk_len, seed, flags, P.shard[r].lo, P.shard[r].hi, F.st[r]));
        GEMHIP_TRY(gemhip_n2v_vocab(h[r].h, F.st[r]));
        void *c = nullptr;
        GEMHIP_TRY(gemhip_n2v_counts_ptr(h[r].h, &c));
        cnt[r] = (int32_t *)c;
    }
    GEMHIP_TRY(F.all_reduce_sum_i32(cnt, n));
    GEMHIP_TRY(F.sync_all());
    // ---- the walk corpus on every rank: shard r occupies rows [r * shard_rows, ...) (shorter shards padded with -1 tokens)
    const size_t shard_bytes = (size_t)P.shard_rows * walk_len * sizeof(int32_t);
    std::vector<void *> cptr(N);
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(alloc_on(corpus[r], F.dev[r], shard_bytes * N));
        char *mine = corpus[r].get() + (size_t)r * shard_bytes;
        if (hipMemsetAsync(mine, 0xff, shard_bytes, F.st[r]) != hipSuccess) return fail(GEMHIP_E_HIP, "n2v_train_multi: memset");
        GEMHIP_TRY(gemhip_n2v_copy_walks(h[r].h, 0, P.shard[r].hi - P.shard[r].lo, mine, F.st[r]));
        cptr[r] = corpus[r].get();
    }
    GEMHIP_TRY(F.all_gather_inplace(cptr, shard_bytes));
    // ---- the per-partition unigram tables, in the layout the flags ask for: node-id order, or (GEMHIP_N2V_VOCAB_ORDER, the plugin default on one GPU)
    // the binary's -- each partition's nodes in order of first appearance in the WHOLE corpus, which every rank now holds
    GEMHIP_TRY(F.sync_all());
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(F.use(r));
        GEMHIP_TRY((flags & GEMHIP_N2V_VOCAB_ORDER) ? gemhip_n2v_build_unigram_parts_vocab_order(h[r].h, N, flags, corpus[r].get(), (int64_t)N * P.shard_rows * walk_len, nullptr, nullptr, nullptr, nullptr)
                                                    : gemhip_n2v_build_unigram_parts(h[r].h, N, nullptr, nullptr));
    }
    // ---- LOCALLY HOT ROWS of the gathered corpus (nodes whose tokens are packed into few walks: the ends of isolated edges): never cached by the bucket launches
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(F.use(r));
        GEMHIP_TRY(gemhip_n2v_locally_hot_corpus(h[r].h, corpus[r].get(), (int64_t)N * P.shard_rows, walk_len, -1, nullptr, F.st[r]));
    }
    // ---- the episode table on every rank; InitPosEmb / InitNegEmb of the whole table a single GPU would draw, once (rank 0's device)
    const size_t part_bytes = (size_t)P.prow * d * sizeof(float);
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(alloc_on(segd[r], F.dev[r], P.tab.size() * sizeof(int64_t)));
        if (hipMemcpy(segd[r].get(), P.tab.data(), P.tab.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) return fail(GEMHIP_E_HIP, "n2v_train_multi: table upload");
        if (r == 0) GEMHIP_TRY(gemhip_sgns_init(h[0].h, d, seed, nullptr, nullptr));
        GEMHIP_TRY(alloc_on(Pp[r], F.dev[r], part_bytes));
        GEMHIP_TRY(alloc_on(Na[r], F.dev[r], part_bytes));
        GEMHIP_TRY(alloc_on(Nb[r], F.dev[r], part_bytes));
    }
    // ---- partition r of those tables: SynPos cut out of a host copy (the handle keeps its tables private; get_tables synchronises the device), SynNeg = 0
    {
        std::vector<float> full((size_t)n * d), part((size_t)P.prow * d);
        GEMHIP_TRY(F.use(0));
        GEMHIP_TRY(gemhip_sgns_get_tables(h[0].h, full.data(), nullptr));
        for (int r = 0; r < N; ++r) {
            partition_cut(full.data(), n, d, r, N, part.data());
            GEMHIP_TRY(F.use(r));
            if (hipMemcpy(Pp[r].get(), part.data(), part_bytes, hipMemcpyHostToDevice) != hipSuccess || hipMemsetAsync(Na[r].get(), 0, part_bytes, F.st[r]) != hipSuccess ||
                hipMemsetAsync(Nb[r].get(), 0, part_bytes, F.st[r]) != hipSuccess)
                return fail(GEMHIP_E_HIP, "n2v_train_multi: partition upload failed on rank %d", r);
        }
    }
    GEMHIP_TRY(F.sync_all());
    const double t1 = now_s();
    // ---- episodes x rounds: bucket (r, (r + s) % N) on rank r, then the SynNeg partitions move one step around the ring
    std::vector<void *> ncur(N), ntmp(N);
    for (int r = 0; r < N; ++r) { ncur[r] = Na[r].get(); ntmp[r] = Nb[r].get(); }
    int64_t launches = 0;
    for (int ep = 0; ep < epochs; ++ep)
        for (int e = 0; e < episodes; ++e)
            for (int s = 0; s < N; ++s) {
                for (int r = 0; r < N; ++r) {
                    GEMHIP_TRY(F.use(r));
                    GEMHIP_TRY(gemhip_sgns_train_part(h[r].h, corpus[r].get(), (int64_t)N * P.seg_len[e], walk_len, (const int64_t *)segd[r].get() + (P.episode(e) - P.episode(0)), N,
                                                      P.seg_len[e], 0, window, 0.025f, P.alpha_total, P.token_offset[(size_t)ep * episodes + e], ep, seed, flags, r, (r + s) % N,
                                                      Pp[r].get(), ncur[r], d, F.st[r]));
                    ++launches;
                }
                if (N > 1) { GEMHIP_TRY(F.ring_shift(ncur, ntmp, part_bytes)); std::swap(ncur, ntmp); }
            }
    GEMHIP_TRY(F.sync_all());
    const double t2 = now_s();
    // ---- the result: every partition pasted back into node-id order
    double pairs = 0;
    std::vector<float> part((size_t)P.prow * d);
    for (int r = 0; r < N; ++r) {
        GEMHIP_TRY(F.use(r));
        if (hipMemcpy(part.data(), Pp[r].get(), part_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(GEMHIP_E_HIP, "n2v_train_multi: download failed on rank %d", r);
        partition_paste(part.data(), n, d, r, N, X_out);
        int64_t pr = 0;
        GEMHIP_TRY(gemhip_sgns_pairs(h[r].h, &pr, 1));
        pairs += (double)pr;
    }
    if (stats) {
        stats[0] = t1 - t0; stats[1] = t2 - t1; stats[2] = (double)total * walk_len; stats[3] = pairs; stats[4] = N > 1 ? (double)part_bytes : 0.0; stats[5] = N;
        stats[6] = F.virt ? 1.0 : 0.0; stats[7] = (double)launches / N;
    }
    return GEMHIP_OK;
}

