// sym_eig.hip -- the host symmetric eigensolver (fp64) behind the HOPE / Laplacian Eigenmaps / LLE solvers of hope_solve.hip; interface: sym_eig.hpp.
// Householder tridiagonalisation + implicit-shift QL (the classical EISPACK tred2/tql2 pair) for the projected eigenproblems (<= 512 x 512), a
// partial solver for the top m pairs, and the host threads of their O(n^3) phases.
// HIP-FREE BY RULE: no HIP header, nothing from common.hpp, no kernel -- the file compiles with plain `clang++ -x c++ -std=c++17` as well as with
// hipcc, which is how scripts/build_tsan_eig.sh puts it under ThreadSanitizer.  It keeps the .hip suffix only so that the `csrc/*.hip` globs of
// the library build and of the sanitizer builds pick it up unchanged.
#include "sym_eig.hpp"
#include <cmath>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <cstdlib>
#include <atomic>
#include <thread>
#include <sched.h>

namespace gemhip {

namespace {

double g_eig_seconds = 0.0, g_eig_calls = 0.0;
sym_eig_cb_t g_eig_cb = nullptr;

static inline double eig_hypot(double a, double b) { const double r = std::sqrt(a * a + b * b); return (r > 1e-150 && r < 1e150) ? r : std::hypot(a, b); }
// Inner loops of the eigensolver, written over contiguous columns with restrict pointers and compiled twice
// (baseline x86-64 and AVX2+FMA, chosen at run time) -- host code only.
#define EIG_KERNELS(SFX, ATTR)                                                                                         \
    ATTR static double eig_dot##SFX(const double *__restrict a, const double *__restrict b, int n)                     \
    {                                                                                                                  \
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;                                                                         \
        int k = 0;                                                                                                     \
        for (; k + 4 <= n; k += 4) { s0 += a[k] * b[k]; s1 += a[k + 1] * b[k + 1]; s2 += a[k + 2] * b[k + 2]; s3 += a[k + 3] * b[k + 3]; } \
        for (; k < n; ++k) s0 += a[k] * b[k];                                                                          \
        return (s0 + s1) + (s2 + s3);                                                                                  \
    }                                                                                                                  \
    ATTR static void eig_axpy##SFX(double *__restrict y, double a, const double *__restrict x, int n)                  \
    {                                                                                                                  \
        for (int k = 0; k < n; ++k) y[k] += a * x[k];                                                                  \
    }                                                                                                                  \
    ATTR static void eig_axpy2##SFX(double *__restrict y, double a, const double *__restrict x, double b, const double *__restrict z, int n) \
    {                                                                                                                  \
        for (int k = 0; k < n; ++k) y[k] -= a * x[k] + b * z[k];                                                       \
    }                                                                                                                  \
    ATTR static void eig_rot##SFX(double *__restrict p0, double *__restrict p1, int n, double c, double s)            \
    {                                                                                                                  \
        for (int k = 0; k < n; ++k) { const double h = p1[k]; p1[k] = s * p0[k] + c * h; p0[k] = c * p0[k] - s * h; }  \
    }                                                                                                                  \
    /* two columns of the symmetric matrix-vector product at once: dots c0.d, c1.d and e += f0 c0 + f1 c1 -- d and e are  \
       loaded once for both columns (5 loads + 1 store per 4 multiply-adds instead of 6 + 2) */                          \
    ATTR static void eig_symv2##SFX(const double *__restrict c0, const double *__restrict c1, const double *__restrict d, \
                                    double *__restrict e, double f0, double f1, int n, double *__restrict out)         \
    {                                                                                                                  \
        double a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, b[8] = {0, 0, 0, 0, 0, 0, 0, 0};                                       \
        int k = 0;                                                                                                     \
        for (; k + 8 <= n; k += 8)                                                                                     \
            for (int u = 0; u < 8; ++u) {                                                                              \
                const double x0 = c0[k + u], x1 = c1[k + u], dk = d[k + u];                                            \
                a[u] += x0 * dk; b[u] += x1 * dk;                                                                      \
                e[k + u] += f0 * x0 + f1 * x1;                                                                         \
            }                                                                                                          \
        for (; k < n; ++k) { const double x0 = c0[k], x1 = c1[k], dk = d[k]; a[0] += x0 * dk; b[0] += x1 * dk; e[k] += f0 * x0 + f1 * x1; } \
        out[0] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));                                    \
        out[1] = ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));                                    \
    }                                                                                                                  \
    /* ... and of the rank-2 update: y0 -= f0 x + g0 z, y1 -= f1 x + g1 z */                                           \
    ATTR static void eig_axpy22##SFX(double *__restrict y0, double *__restrict y1, const double *__restrict x, const double *__restrict z, \
                                     double f0, double g0, double f1, double g1, int n)                                \
    {                                                                                                                  \
        for (int k = 0; k < n; ++k) { const double xk = x[k], zk = z[k]; y0[k] -= f0 * xk + g0 * zk; y1[k] -= f1 * xk + g1 * zk; } \
    }
EIG_KERNELS(_base, )
EIG_KERNELS(_avx2, __attribute__((target("avx2,fma"))))
EIG_KERNELS(_avx512, __attribute__((target("avx512f,avx512dq,avx512vl,fma"))))
#undef EIG_KERNELS

struct EigOps {
    double (*dot)(const double *, const double *, int);
    void (*axpy)(double *, double, const double *, int);
    void (*axpy2)(double *, double, const double *, double, const double *, int);
    void (*rot)(double *, double *, int, double, double);
    void (*symv2)(const double *, const double *, const double *, double *, double, double, int, double *);
    void (*axpy22)(double *, double *, const double *, const double *, double, double, double, double, int);
};
// Which build of the inner loops this host runs: GEMHIP_EIG_ISA=base|avx2|avx512 forces one (if the CPU has it); otherwise the widest the CPU
// supports -- AVX-512 only where it is actually faster on THIS host (a 512-bit unit that is double-pumped, or a core that drops its clock for
// 512-bit work, gains nothing): decided once by timing the reduction's two hot loops (dot + axpy over 2 048 doubles, ~50 us in total).
static const EigOps &eig_ops()
{
    static const EigOps base = {eig_dot_base, eig_axpy_base, eig_axpy2_base, eig_rot_base, eig_symv2_base, eig_axpy22_base};
    static const EigOps avx2 = {eig_dot_avx2, eig_axpy_avx2, eig_axpy2_avx2, eig_rot_avx2, eig_symv2_avx2, eig_axpy22_avx2};
    static const EigOps avx512 = {eig_dot_avx512, eig_axpy_avx512, eig_axpy2_avx512, eig_rot_avx512, eig_symv2_avx512, eig_axpy22_avx512};
    static const EigOps *chosen = []() -> const EigOps * {
        const bool has2 = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
        const bool has512 = has2 && __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512dq") && __builtin_cpu_supports("avx512vl");
        if (const char *e = getenv("GEMHIP_EIG_ISA")) {
            if (!strcmp(e, "base")) return &base;
            if (!strcmp(e, "avx2") && has2) return &avx2;
            if (!strcmp(e, "avx512") && has512) return &avx512;
        }
        if (!has2) return &base;
        if (!has512) return &avx2;
        std::vector<double> x(2048), y(2048, 0.0);
        for (int k = 0; k < 2048; ++k) x[k] = 1.0 / (1.0 + k);
        auto time_ops = [&](const EigOps &op) {
            double best = 1e30, sink = 0.0;
            for (int rep = 0; rep < 5; ++rep) {
                const auto t0 = std::chrono::steady_clock::now();
                for (int it = 0; it < 16; ++it) { sink += op.dot(x.data(), y.data(), 2048); op.axpy(y.data(), 1e-9, x.data(), 2048); op.axpy2(y.data(), 1e-9, x.data(), 1e-9, x.data(), 2048); }
                best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
            }
            return best + (sink == 12345.678 ? 1.0 : 0.0);
        };
        const double t2 = time_ops(avx2), t5 = time_ops(avx512);
        return t5 < 0.9 * t2 ? &avx512 : &avx2;
    }();
    return *chosen;
}

// Host threads for the O(n^3) phases of the eigensolver (the reduction's matrix-vector product and rank-2 update, the
// back-transformation of the wanted vectors).  GEMHIP_EIG_THREADS (read once) or gemhip_set_host_threads(); default 1 (see below), never more
// than half the cores this process may run on.  Threads are created per call and joined before it returns: nothing outlives
// the call, so fork() in the host program (bench.py's CPU baselines are subprocesses) never meets a live pool.
static std::atomic<int> g_eig_threads{-1};       // (atomic: gemhip_set_host_threads may run beside a solve; every phase reads its T once)
static int eig_threads()
{
    int cur = g_eig_threads.load(std::memory_order_relaxed);
    if (cur < 0) {
        // default ONE thread: on the MI355X host the threaded reduction measured SLOWER than one core (directed SBM 100k/1M solve, 9 projected
        // 448 x 448 problems: 39.7 ms of host eigensolves at 1 thread, 52.8 ms at 4 -- profiles/r04_hope_directed_eig_threads.json; the spin
        // barriers of a ~3 us step lose to the host's scheduling noise; the build container measured 1.8x FASTER at 4).  GEMHIP_EIG_THREADS opts in.
        int t = 1;
        if (const char *e = getenv("GEMHIP_EIG_THREADS")) t = atoi(e);
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0) t = std::min(t, std::max(1, CPU_COUNT(&set) / 2));   // spin barriers want idle cores
        cur = std::max(1, std::min(t, 16));
        g_eig_threads.store(cur, std::memory_order_relaxed);
    }
    return cur;
}

// Sense-reversing barrier: a step of the reduction is a few microseconds of work per thread, far below what a futex
// round trip costs, so waiters spin (and yield once the wait is long: an oversubscribed host must not live-lock).
struct SpinBarrier {
    std::atomic<int> count{0}, gen{0};
    int T = 1;
    void wait()
    {
        const int g = gen.load(std::memory_order_acquire);
        if (count.fetch_add(1, std::memory_order_acq_rel) == T - 1) {
            count.store(0, std::memory_order_relaxed);
            gen.store(g + 1, std::memory_order_release);
            return;
        }
        for (int spins = 0; gen.load(std::memory_order_acquire) == g; ++spins) {
            if (spins < 2048) {
#if !defined(__HIP_DEVICE_COMPILE__)       // the library build compiles this file as HIP, whose device pass parses host functions too and has no x86 builtins
                __builtin_ia32_pause();
#endif
            } else std::this_thread::yield();
        }
    }
};

// Householder reduction to tridiagonal form (the first half of tred2), column-major access.  On return: the diagonal of T
// is A(i,i), e[i] (i >= 1) couples i-1 and i, column i+1 rows 0..i hold the reflector u_{i+1} and d[i+1] its h = |u|^2/2
// (0: no reflector), so that  Q = P_{n-1} ... P_1,  P_i = I - u_i u_i^T / h_i  on the leading i coordinates.
// eig_reduce_steps runs steps i = i_from .. 1; on entry d[0..i_from) holds row i_from of the current matrix.
static void eig_reduce_steps(int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e, const EigOps &op, int i_from)
{
    auto A = [&](int i, int j) -> double & { return V[(size_t)j * n + i]; };
    auto col = [&](int j) -> double * { return V.data() + (size_t)j * n; };
    for (int i = i_from; i > 0; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) scale += std::fabs(d[k]);
        if (scale == 0.0) {
            e[i] = d[i - 1];
            for (int j = 0; j < i; ++j) { d[j] = A(i - 1, j); A(i, j) = 0.0; A(j, i) = 0.0; }
        } else {
            for (int k = 0; k < i; ++k) { d[k] /= scale; h += d[k] * d[k]; }
            double f = d[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            e[i] = scale * g;
            h -= f * g;
            d[i - 1] = f - g;
            for (int j = 0; j < i; ++j) e[j] = 0.0;
            int j = 0;
            static const bool pairs = !(getenv("GEMHIP_EIG_PAIRS") && atoi(getenv("GEMHIP_EIG_PAIRS")) == 0);
            for (; pairs && j + 1 < i; j += 2) {              // columns j and j + 1 together (eig_symv2: d and e travel once for both)
                const double f0 = d[j], f1 = d[j + 1];
                A(j, i) = f0; A(j + 1, i) = f1;
                double g0 = e[j] + A(j, j) * f0;
                const double a = A(j + 1, j);                 // column j's first element below the diagonal belongs to column j alone
                g0 += a * f1;
                e[j + 1] += f0 * a;
                double g1 = e[j + 1] + A(j + 1, j + 1) * f1;
                const int len = i - 2 - j;                    // k = j+2 .. i-1
                if (len > 0) {
                    double s2[2];
                    op.symv2(col(j) + j + 2, col(j + 1) + j + 2, d.data() + j + 2, e.data() + j + 2, f0, f1, len, s2);
                    g0 += s2[0]; g1 += s2[1];
                }
                e[j] = g0; e[j + 1] = g1;
            }
            for (; j < i; ++j) {
                f = d[j];
                A(j, i) = f;
                g = e[j] + A(j, j) * f;
                const int len = i - 1 - j;                    // k = j+1 .. i-1
                if (len > 0) {
                    g += op.dot(col(j) + j + 1, d.data() + j + 1, len);
                    op.axpy(e.data() + j + 1, f, col(j) + j + 1, len);
                }
                e[j] = g;
            }
            f = 0.0;
            for (int jj = 0; jj < i; ++jj) { e[jj] /= h; f += e[jj] * d[jj]; }
            const double hh = f / (h + h);
            for (int jj = 0; jj < i; ++jj) e[jj] -= hh * d[jj];
            j = 0;
            for (; pairs && j + 1 < i; j += 2) {
                const double f0 = d[j], g0 = e[j], f1 = d[j + 1], g1 = e[j + 1];
                A(j, j) -= f0 * g0 + g0 * f0;                 // k = j of column j
                op.axpy22(col(j) + j + 1, col(j + 1) + j + 1, e.data() + j + 1, d.data() + j + 1, f0, g0, f1, g1, i - j - 1);     // k = j+1 .. i-1 of both
                d[j] = A(i - 1, j); d[j + 1] = A(i - 1, j + 1);
                A(i, j) = 0.0; A(i, j + 1) = 0.0;
            }
            for (; j < i; ++j) {
                f = d[j]; g = e[j];
                op.axpy2(col(j) + j, f, e.data() + j, g, d.data() + j, i - j);     // k = j .. i-1
                d[j] = A(i - 1, j);
                A(i, j) = 0.0;
            }
        }
        d[i] = h;
    }
}

// The same steps i = n-1 .. i_stop on T threads.  Columns are dealt to the threads in blocks of 8 (block-cyclic: the
// active triangle shrinks from the right, so every thread keeps an equal share, and a thread always meets the same
// columns -- they stay in its own L2).  Per step: every thread forms the scaled reflector from the shared row (O(i),
// redundantly, on a private copy), computes its columns' share of p = A u into a private partial vector (the lower
// triangle is read once: dot for the part below the diagonal, axpy for the mirrored part), BARRIER, sums the partials
// (O(T i), redundantly), applies the rank-2 update to its own columns and publishes the elements of the next row it
// owns, BARRIER.  Two barriers and no shared writes besides those rows; sums are taken in a different order than the
// serial loop takes them, so results agree to rounding (1e-16 relative), not bit for bit.
// Returns the last step it completed (i_stop, or an earlier one: thread 0 times every 8 steps against what ONE thread would
// need at a pessimistic 4 GFLOP/s and calls the threaded phase off when it is not even keeping up with that -- the sign of
// a host whose cores are taken (another library's worker threads spinning after a BLAS call make every barrier cost a
// scheduler quantum: measured 110 ms instead of 5 ms for n = 448 on an 8-core container).  The caller finishes the steps down to i_stop with
// eig_reduce_virtual (the same arithmetic on one thread), so WHEN the threads were called off never shows in the result.
static int eig_reduce_mt(int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e, const EigOps &op, int T, int i_stop)
{
    std::atomic<int> bail{0}, go{0};
    int i_done = n;
    const char *tb = getenv("GEMHIP_EIG_TEST_BAIL_AFTER");       // test hook: call the threaded phase off after this many steps
    const int test_bail_after = tb ? atoi(tb) : -1;
    const int CB = 8;                                            // column block = one cache line of the shared row
    const size_t ldp = ((size_t)n + 15) / 8 * 8 + 8;
    std::vector<double> parts((size_t)T * ldp, 0.0), rows(2 * ldp, 0.0);
    for (int j = 0; j < n; ++j) rows[j] = d[j];
    SpinBarrier bar; bar.T = T;
    auto body = [&](int t) {
        auto A = [&](int i, int j) -> double & { return V[(size_t)j * n + i]; };
        auto col = [&](int j) -> double * { return V.data() + (size_t)j * n; };
        std::vector<double> dl(n, 0.0), el(n, 0.0);
        double *mine = parts.data() + (size_t)t * ldp;
        double *cur = rows.data(), *nxt = rows.data() + ldp;
        if (t > 0) {                                             // workers wait for the verdict on thread creation (1 run, 2 abort)
            for (int spins = 0; go.load(std::memory_order_acquire) == 0; ++spins)
                if (spins > 2048) std::this_thread::yield();
            if (go.load(std::memory_order_acquire) == 2) return;
        }
        bar.wait();                                              // everybody is up: thread start-up stays out of the timing below
        auto tick = std::chrono::steady_clock::now();
        double budget = 0.0;                                     // seconds one thread would need for the steps since `tick`
        auto end_of_step = [&](int i) {                          // thread 0, right before the barrier that ends step i
            if (test_bail_after >= 0 && n - 1 - i >= test_bail_after) bail.store(1, std::memory_order_relaxed);
            budget += 4.0 * i * i / 4e9 + 1e-6;
            if (n - 1 - i < 8 || ((n - 1 - i) & 7) == 7) {        // every step at first: a contended host shows at the first barrier
                const auto now = std::chrono::steady_clock::now();
                if (std::chrono::duration<double>(now - tick).count() > budget) bail.store(1, std::memory_order_relaxed);
                tick = now; budget = 0.0;
            }
        };
        int i = n - 1;
        for (; i >= i_stop; --i) {
            if (bail.load(std::memory_order_relaxed)) break;    // stored before the barrier that ended step i+1: all threads agree
            double scale = 0.0, h = 0.0;
            for (int k = 0; k < i; ++k) { dl[k] = cur[k]; scale += std::fabs(dl[k]); }
            if (scale == 0.0) {
                if (t == 0) { e[i] = dl[i - 1]; d[i] = 0.0; }
                bar.wait();      // two barriers in this branch as well: thread 0 raises `bail` between the two barriers of a step, and every
                                 // thread reads it after the second one -- with a single barrier a late thread could read it a step early
                for (int jb = t * CB; jb < i; jb += T * CB)
                    for (int j = jb; j < std::min(jb + CB, i); ++j) { nxt[j] = A(i - 1, j); A(i, j) = 0.0; A(j, i) = 0.0; }
                if (t == 0) end_of_step(i);
                bar.wait();
                std::swap(cur, nxt);
                continue;
            }
            for (int k = 0; k < i; ++k) { dl[k] /= scale; h += dl[k] * dl[k]; }
            double f = dl[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            if (t == 0) e[i] = scale * g;
            h -= f * g;
            dl[i - 1] = f - g;
            for (int k = 0; k < i; ++k) mine[k] = 0.0;
            for (int jb = t * CB; jb < i; jb += T * CB)
                for (int j = jb; j < std::min(jb + CB, i); ++j) {
                    f = dl[j];
                    A(j, i) = f;
                    g = A(j, j) * f;
                    const int len = i - 1 - j;
                    if (len > 0) {
                        g += op.dot(col(j) + j + 1, dl.data() + j + 1, len);
                        op.axpy(mine + j + 1, f, col(j) + j + 1, len);
                    }
                    mine[j] += g;
                }
            bar.wait();
            for (int k = 0; k < i; ++k) el[k] = parts[k];
            for (int u = 1; u < T; ++u) {
                const double *pu = parts.data() + (size_t)u * ldp;
                for (int k = 0; k < i; ++k) el[k] += pu[k];
            }
            f = 0.0;
            for (int j = 0; j < i; ++j) { el[j] /= h; f += el[j] * dl[j]; }
            const double hh = f / (h + h);
            for (int j = 0; j < i; ++j) el[j] -= hh * dl[j];
            for (int jb = t * CB; jb < i; jb += T * CB)
                for (int j = jb; j < std::min(jb + CB, i); ++j) {
                    op.axpy2(col(j) + j, dl[j], el.data() + j, el[j], dl.data() + j, i - j);
                    nxt[j] = A(i - 1, j);
                    A(i, j) = 0.0;
                }
            if (t == 0) { d[i] = h; end_of_step(i); }
            bar.wait();
            std::swap(cur, nxt);
        }
        if (t == 0) {
            i_done = i + 1;
            for (int k = 0; k < i_done; ++k) d[k] = cur[k];       // the state eig_reduce_steps continues from
        }
    };
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < T; ++t) pool.emplace_back(body, t);
    } catch (...) {                                              // no more threads to be had (pid limit, memory): the caller's serial loop does it all
        go.store(2, std::memory_order_release);
        for (auto &th : pool) th.join();
        for (int k = 0; k < n; ++k) d[k] = rows[k];
        return n;
    }
    go.store(1, std::memory_order_release);
    const auto t1 = std::chrono::steady_clock::now();
    body(0);
    const auto t2 = std::chrono::steady_clock::now();
    for (auto &th : pool) th.join();
    if (getenv("GEMHIP_EIG_DEBUG")) {
        auto ms = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
        fprintf(stderr, "[eig-mt] n=%d T=%d create %.3f ms  steps %d..%d %.3f ms  join %.3f ms\n", n, T, ms(t0, t1), n - 1, i_done, ms(t1, t2),
                ms(t2, std::chrono::steady_clock::now()));
    }
    return i_done;
}

// Steps i_from .. i_stop with the ARITHMETIC of eig_reduce_mt at T threads, on the calling thread: the same columns feed the same partial
// vectors in the same order and the partials are summed in the same order, so the result is bit-identical to what the T threads would have
// produced.  This is what continues after eig_reduce_mt called its threads off (or could not create them): the output of the reduction then
// depends on T alone, never on when the contended-host check fired.
static void eig_reduce_virtual(int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e, const EigOps &op, int T, int i_from, int i_stop)
{
    const int CB = 8;
    const size_t ldp = ((size_t)n + 15) / 8 * 8 + 8;
    std::vector<double> parts((size_t)T * ldp, 0.0), dl(n, 0.0), el(n, 0.0), nxt(n, 0.0);
    auto A = [&](int i, int j) -> double & { return V[(size_t)j * n + i]; };
    auto col = [&](int j) -> double * { return V.data() + (size_t)j * n; };
    for (int i = i_from; i >= i_stop; --i) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; ++k) { dl[k] = d[k]; scale += std::fabs(dl[k]); }
        if (scale == 0.0) {
            e[i] = dl[i - 1];
            for (int j = 0; j < i; ++j) { nxt[j] = A(i - 1, j); A(i, j) = 0.0; A(j, i) = 0.0; }
            for (int j = 0; j < i; ++j) d[j] = nxt[j];
            d[i] = 0.0;
            continue;
        }
        for (int k = 0; k < i; ++k) { dl[k] /= scale; h += dl[k] * dl[k]; }
        double f = dl[i - 1];
        double g = std::sqrt(h);
        if (f > 0) g = -g;
        e[i] = scale * g;
        h -= f * g;
        dl[i - 1] = f - g;
        for (int t = 0; t < T; ++t) {
            double *mine = parts.data() + (size_t)t * ldp;
            for (int k = 0; k < i; ++k) mine[k] = 0.0;
            for (int jb = t * CB; jb < i; jb += T * CB)
                for (int j = jb; j < std::min(jb + CB, i); ++j) {
                    f = dl[j];
                    A(j, i) = f;
                    g = A(j, j) * f;
                    const int len = i - 1 - j;
                    if (len > 0) {
                        g += op.dot(col(j) + j + 1, dl.data() + j + 1, len);
                        op.axpy(mine + j + 1, f, col(j) + j + 1, len);
                    }
                    mine[j] += g;
                }
        }
        for (int k = 0; k < i; ++k) el[k] = parts[k];
        for (int u = 1; u < T; ++u) {
            const double *pu = parts.data() + (size_t)u * ldp;
            for (int k = 0; k < i; ++k) el[k] += pu[k];
        }
        f = 0.0;
        for (int j = 0; j < i; ++j) { el[j] /= h; f += el[j] * dl[j]; }
        const double hh = f / (h + h);
        for (int j = 0; j < i; ++j) el[j] -= hh * dl[j];
        for (int j = 0; j < i; ++j) {
            op.axpy2(col(j) + j, dl[j], el.data() + j, el[j], dl.data() + j, i - j);
            nxt[j] = A(i - 1, j);
            A(i, j) = 0.0;
        }
        for (int j = 0; j < i; ++j) d[j] = nxt[j];
        d[i] = h;
    }
}

static void eig_reduce(int n, std::vector<double> &V, std::vector<double> &d, std::vector<double> &e, const EigOps &op)
{
    for (int j = 0; j < n; ++j) d[j] = V[(size_t)j * n + (n - 1)];
    const int T = eig_threads();
    int i_from = n - 1;
    const int i_stop = 96;                     // below this a step is shorter than its two barriers
    if (T > 1 && n >= 2 * i_stop) {
        const int i_done = eig_reduce_mt(n, V, d, e, op, T, i_stop);
        if (i_done > i_stop) eig_reduce_virtual(n, V, d, e, op, T, i_done - 1, i_stop);    // threads called off early: same arithmetic, one thread
        i_from = i_stop - 1;
    }
    eig_reduce_steps(n, V, d, e, op, i_from);
}

}  // namespace

void sym_eig_impl(int n, std::vector<double> &V, std::vector<double> &d)
{
    const EigOps &op = eig_ops();
    std::vector<double> e(n, 0.0);
    d.assign(n, 0.0);
    const bool eig_dbg = getenv("GEMHIP_EIG_DEBUG") != nullptr;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto tA = tnow();
    // column-major accessor: every O(n^3) loop below runs over the FIRST index, i.e. contiguous memory
    // (the input is symmetric, so its layout does not matter; the result is transposed back at the end)
    auto A = [&](int i, int j) -> double & { return V[(size_t)j * n + i]; };
    auto col = [&](int j) -> double * { return V.data() + (size_t)j * n; };
    eig_reduce(n, V, d, e, op);
    auto tB = tnow();
    for (int i = 0; i < n - 1; ++i) {
        A(n - 1, i) = A(i, i);
        A(i, i) = 1.0;
        const double h = d[i + 1];
        if (h != 0.0) {
            for (int k = 0; k <= i; ++k) d[k] = A(k, i + 1) / h;
            for (int j = 0; j <= i; ++j) {
                const double g = op.dot(col(i + 1), col(j), i + 1);
                op.axpy(col(j), -g, d.data(), i + 1);
            }
        }
        for (int k = 0; k <= i; ++k) A(k, i + 1) = 0.0;
    }
    for (int j = 0; j < n; ++j) { d[j] = A(n - 1, j); A(n - 1, j) = 0.0; }
    A(n - 1, n - 1) = 1.0;
    e[0] = 0.0;
    auto tC = tnow();
    // QL
    for (int i = 1; i < n; ++i) e[i - 1] = e[i];
    e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::pow(2.0, -52.0);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n) { if (std::fabs(e[m]) <= eps * tst1) break; ++m; }
        if (m > l) {
            int iter = 0;
            do {
                ++iter;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = eig_hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                    op.rot(col(i), col(i + 1), n, c, s);
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1 && iter < 200);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    if (eig_dbg) { auto tD = tnow(); auto ms = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count() * 1e3; };
        fprintf(stderr, "[eig] n=%d reduce %.2f ms  accumulate %.2f ms  ql %.2f ms\n", n, ms(tA, tB), ms(tB, tC), ms(tC, tD)); }
    for (int i = 0; i < n - 1; ++i) {                   // sort ascending
        int k = i; double p = d[i];
        for (int j = i + 1; j < n; ++j) if (d[j] < p) { k = j; p = d[j]; }
        if (k != i) {
            d[k] = d[i]; d[i] = p;
            for (int j = 0; j < n; ++j) std::swap(A(j, i), A(j, k));
        }
    }
    for (int i = 0; i < n; ++i)                              // back to row-major: V[i*n + j] = component i of eigenvector j
        for (int j = i + 1; j < n; ++j) std::swap(V[(size_t)i * n + j], V[(size_t)j * n + i]);
}

// Eigenvalues of the symmetric tridiagonal (diag a, a[i]~a[i+1] coupled by b[i]) by implicit QL without vectors: O(n^2).
static void tridiag_eigenvalues(int n, std::vector<double> d, std::vector<double> e, std::vector<double> &w)
{
    // d: diagonal; e[i] couples i and i+1 (e[n-1] = 0), the layout tql2 above uses after its shift
    e.resize(n, 0.0); e[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = std::pow(2.0, -52.0);
    for (int l = 0; l < n; ++l) {
        tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
        int m = l;
        while (m < n) { if (std::fabs(e[m]) <= eps * tst1) break; ++m; }
        if (m > l) {
            int iter = 0;
            do {
                ++iter;
                double g = d[l];
                double p = (d[l + 1] - g) / (2.0 * e[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                d[l] = e[l] / (p + r);
                d[l + 1] = e[l] * (p + r);
                const double dl1 = d[l + 1];
                double h = g - d[l];
                for (int i = l + 2; i < n; ++i) d[i] -= h;
                f += h;
                p = d[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = e[l + 1];
                for (int i = m - 1; i >= l; --i) {
                    c3 = c2; c2 = c; s2 = s;
                    g = c * e[i];
                    h = c * p;
                    r = eig_hypot(p, e[i]);
                    e[i + 1] = s * r;
                    s = e[i] / r;
                    c = p / r;
                    p = c * d[i] - s * g;
                    d[i + 1] = h + s * (c * g + s * d[i]);
                }
                p = -s * s2 * c3 * el1 * e[l] / dl1;
                e[l] = s * p;
                d[l] = c * p;
            } while (std::fabs(e[l]) > eps * tst1 && iter < 200);
        }
        d[l] += f;
        e[l] = 0.0;
    }
    std::sort(d.begin(), d.end());
    w = d;
}

// The m LARGEST eigenpairs of a symmetric matrix: Householder reduction, eigenvalues of the tridiagonal by QL, the m
// eigenvectors by inverse iteration (LU with partial pivoting of T - lambda I, close eigenvalues re-orthogonalised as one
// cluster -- the scheme of LAPACK's dstein), then the reflectors applied to those m vectors only.  2/3 n^3 + O(n^2 m)
// flops instead of the ~5 n^3 of the full solver: the Rayleigh-Ritz step of the Krylov solver only ever uses the leading
// block of Ritz vectors.  A (n x n row-major symmetric) is destroyed; w: m eigenvalues DESCENDING; Z: column-major n x m.
void sym_eig_top_impl(int n, std::vector<double> &V, int m, std::vector<double> &w, std::vector<double> &Z)
{
    const EigOps &op = eig_ops();
    std::vector<double> d(n, 0.0), e(n, 0.0);
    const bool eig_dbg = getenv("GEMHIP_EIG_DEBUG") != nullptr;
    auto tnow = [] { return std::chrono::steady_clock::now(); };
    auto tms = [](auto x, auto y) { return std::chrono::duration<double>(y - x).count() * 1e3; };
    const auto tA = tnow();
    eig_reduce(n, V, d, e, op);
    const auto tB = tnow();
    auto col = [&](int j) -> double * { return V.data() + (size_t)j * n; };
    std::vector<double> a(n), b(n, 0.0), hh(d);                      // T: diagonal a, b[i] couples i, i+1 ; hh[i] = h of reflector i
    for (int i = 0; i < n; ++i) a[i] = V[(size_t)i * n + i];
    for (int i = 0; i + 1 < n; ++i) b[i] = e[i + 1];
    std::vector<double> all;
    tridiag_eigenvalues(n, a, b, all);                                // ascending
    const auto tC = tnow();
    double norm = 0.0;
    for (int i = 0; i < n; ++i) norm = std::max(norm, std::fabs(a[i]) + (i ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < n ? std::fabs(b[i]) : 0.0));
    const double eps = std::pow(2.0, -52.0);
    const double tiny = std::max(eps * norm, 1e-300), ortol = 1e-3 * norm, pert = 10.0 * eps * norm;
    w.assign(m, 0.0);
    Z.assign((size_t)n * m, 0.0);
    std::vector<double> p(n), q(n), r(n), mult(n), x(n);
    std::vector<char> swp(n);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (double)((rng >> 11) & 0xFFFFFFFFFFFFFull) / 4503599627370496.0 * 2.0 - 1.0; };
    double prev_shift = 0.0;
    int cluster0 = 0;
    for (int j = 0; j < m; ++j) {
        const double lam_true = all[n - 1 - j];
        w[j] = lam_true;
        double lam = lam_true;
        if (j > 0 && prev_shift - lam < pert) lam = prev_shift - pert;               // identical shifts would give identical vectors
        if (j == 0 || all[n - j] - lam_true > ortol) cluster0 = j;                    // gap to the previous eigenvalue opens a new cluster
        prev_shift = lam;
        // LU of T - lam I with row interchanges: row i becomes [p, q, r], multiplier mult[i] applied to the row below
        double u = a[0] - lam, v = n > 1 ? b[0] : 0.0;
        for (int i = 0; i + 1 < n; ++i) {
            const double sub = b[i], nd = a[i + 1] - lam, nsup = i + 2 < n ? b[i + 1] : 0.0;
            if (std::fabs(sub) > std::fabs(u)) {
                swp[i] = 1; mult[i] = u / sub; p[i] = sub; q[i] = nd; r[i] = nsup;
                u = v - mult[i] * nd; v = -mult[i] * nsup;
            } else {
                if (u == 0.0) u = tiny;
                swp[i] = 0; mult[i] = sub / u; p[i] = u; q[i] = v; r[i] = 0.0;
                u = nd - mult[i] * v; v = nsup;
            }
        }
        p[n - 1] = u; q[n - 1] = 0.0; r[n - 1] = 0.0;
        for (int i = 0; i < n; ++i) { if (std::fabs(p[i]) < tiny) p[i] = p[i] < 0 ? -tiny : tiny; p[i] = 1.0 / p[i]; }
        for (int i = 0; i < n; ++i) x[i] = rnd();
        double *zj = Z.data() + (size_t)j * n;
        for (int it = 0; it < 5; ++it) {
            for (int i = 0; i + 1 < n; ++i) {                                         // forward: the recorded row operations
                if (swp[i]) { const double t = x[i]; x[i] = x[i + 1]; x[i + 1] = t - mult[i] * x[i]; }
                else x[i + 1] -= mult[i] * x[i];
            }
            for (int i = n - 1; i >= 0; --i) {                                        // back substitution, two super-diagonals
                double t = x[i];
                if (i + 1 < n) t -= q[i] * x[i + 1];
                if (i + 2 < n) t -= r[i] * x[i + 2];
                x[i] = t * p[i];
            }
            double big = 0.0;
            for (int i = 0; i < n; ++i) big = std::max(big, std::fabs(x[i]));
            if (!(big > 0.0) || !std::isfinite(big)) { for (int i = 0; i < n; ++i) x[i] = rnd(); continue; }
            for (int i = 0; i < n; ++i) x[i] /= big;                                  // keeps the next products in range
            for (int c = cluster0; c < j; ++c) {                                      // modified Gram-Schmidt inside the cluster
                const double *zc = Z.data() + (size_t)c * n;
                op.axpy(x.data(), -op.dot(zc, x.data(), n), zc, n);
            }
            const double nrm = std::sqrt(op.dot(x.data(), x.data(), n));
            if (!(nrm > 1e-8)) { for (int i = 0; i < n; ++i) x[i] = rnd(); continue; }   // fell into the span of the cluster: restart
            for (int i = 0; i < n; ++i) x[i] /= nrm;
            if (it >= 2 && big > 0.0) { /* three solves from a random start: converged to working precision */ if (it >= 2) break; }
        }
        std::copy(x.begin(), x.end(), zj);
    }
    const auto tD = tnow();
    // eigenvectors of A = Q z :  apply P_1, ..., P_{n-1} in that order (P_{i+1} acts on coordinates 0..i)
    // (reflector outermost: it stays in L1 while the vectors of a chunk pass under it; chunks of vectors on threads -- every
    // vector sees the same operations in the same order as in a vector-by-vector loop, so the result does not depend on T)
    auto back = [&](int j0, int j1) {
        for (int i = 0; i + 1 < n; ++i) {
            const double h = hh[i + 1];
            if (h == 0.0) continue;
            const double *c = col(i + 1);
            for (int j = j0; j < j1; ++j) {
                double *zj = Z.data() + (size_t)j * n;
                op.axpy(zj, -op.dot(c, zj, i + 1) / h, c, i + 1);
            }
        }
    };
    {
        const int T = (n >= 128 && m >= 8) ? std::min(eig_threads(), m / 4) : 1;
        std::vector<std::thread> pool;
        int started = 1;                                         // chunks handed out (chunk 0 is this thread's)
        try {
            for (int t = 1; t < T; ++t, ++started) pool.emplace_back(back, (int)((int64_t)m * t / T), (int)((int64_t)m * (t + 1) / T));
        } catch (...) {}                                         // thread creation failed: the chunks not handed out are done here
        back(0, T > 1 ? m / T : m);
        for (int t = started; t < T; ++t) back((int)((int64_t)m * t / T), (int)((int64_t)m * (t + 1) / T));
        for (auto &th : pool) th.join();
    }
    if (eig_dbg) fprintf(stderr, "[eig-top] n=%d m=%d reduce %.2f ms  eigenvalues %.2f ms  inverse iteration %.2f ms  back-transform %.2f ms\n", n, m,
                         tms(tA, tB), tms(tB, tC), tms(tC, tD), tms(tD, tnow()));
}

void sym_eig(int n, std::vector<double> &V, std::vector<double> &d)
{
    const auto t0 = std::chrono::steady_clock::now();
    d.assign(n, 0.0);
    if (!(g_eig_cb && n >= 64 && g_eig_cb(n, V.data(), d.data()) == 0)) sym_eig_impl(n, V, d);
    g_eig_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    g_eig_calls += 1.0;
}

// Top-m eigenpairs for the Rayleigh-Ritz step (w descending, Z column-major n x m); small or nearly-full requests and a
// host-supplied solver go through the full decomposition.
void sym_eig_top(int n, std::vector<double> &G, int m, std::vector<double> &w, std::vector<double> &Z)
{
    static const bool no_partial = getenv("GEMHIP_EIG_FULL") != nullptr;
    if (g_eig_cb || no_partial || n < 96 || 2 * m > n) {
        std::vector<double> ev;
        sym_eig(n, G, ev);
        w.assign(m, 0.0); Z.assign((size_t)n * m, 0.0);
        for (int j = 0; j < m; ++j) {
            w[j] = ev[n - 1 - j];
            for (int i = 0; i < n; ++i) Z[(size_t)j * n + i] = G[(size_t)i * n + (n - 1 - j)];
        }
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    sym_eig_top_impl(n, G, m, w, Z);
    g_eig_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    g_eig_calls += 1.0;
}

void set_sym_eig_callback(sym_eig_cb_t fn) { g_eig_cb = fn; }

void set_eig_threads(int threads) { g_eig_threads.store(threads >= 1 ? threads : -1, std::memory_order_relaxed); }
int eig_threads_in_effect() { return eig_threads(); }

void reset_eig_stats() { g_eig_seconds = 0.0; g_eig_calls = 0.0; }
double eig_seconds() { return g_eig_seconds; }
double eig_calls() { return g_eig_calls; }

}  // namespace gemhip
