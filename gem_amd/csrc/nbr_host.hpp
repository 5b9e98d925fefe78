// nbr_host.hpp -- the device-free half of the neighbourhood link-prediction scores (nbr_host.hip): the simple undirected
// CSR of an arc list, the two weight tables, the input checks and the planner that cuts pairs into work items.
// Plain C++, no HIP: everything here runs on a CPU (tests/test_link_heuristics.py); nbr.hip uploads and launches.
#pragma once
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NBR_HD __host__ __device__ inline
#else
#define NBR_HD inline
#endif

namespace gemhip {

// The three constants can be set on the compiler's command line for an A/B build (scripts/bench_link_baselines.py --ab-libs); the tests pin
// the defaults.
#ifndef GEMHIP_NBR_LANES
#define GEMHIP_NBR_LANES 16
#endif
#ifndef GEMHIP_NBR_NARROW
#define GEMHIP_NBR_NARROW 32
#endif
#ifndef GEMHIP_NBR_CHUNK
#define GEMHIP_NBR_CHUNK 2048
#endif
constexpr int NBR_LANES = GEMHIP_NBR_LANES;      // lanes of the group that takes one narrow item (four items per wave)
constexpr int NBR_NARROW = GEMHIP_NBR_NARROW;    // an item of at most this many elements of the shorter list is narrow
constexpr int NBR_CHUNK = GEMHIP_NBR_CHUNK;      // a shorter list above this is cut into slices of this many elements
static_assert(NBR_LANES >= 1 && NBR_LANES <= 64 && (NBR_LANES & (NBR_LANES - 1)) == 0, "a narrow group is a power-of-two share of a wavefront");
static_assert(NBR_NARROW >= 1 && NBR_NARROW <= NBR_CHUNK, "a narrow item is at most one slice");
enum { NBR_CN = 1, NBR_JACCARD = 2, NBR_AA = 4, NBR_RA = 8, NBR_PA = 16, NBR_ALL = 31 };

// Which endpoint's list is searched FOR (a, the shorter) and which is searched IN (b): on equal lengths a is the list of the smaller id, so
// (u, v) and (v, u) walk the same lists in the same order.  Shared with the device: one rule.
NBR_HD bool nbr_first_is_a(int32_t du, int32_t dv, int32_t u, int32_t v) { return du < dv || (du == dv && u < v); }

struct alignas(16) NbrItem {           // 16 bytes, one load
    int32_t pair;                      // index into st / ed
    int32_t start, len;                // the slice of a: elements [start, start + len)
    int32_t slot;                      // -1: the pair is this one item and finishes in place; else the partial slot of this slice
};
struct NbrSplit { int32_t pair, first_slot, n_slots; };

struct NbrPlan {
    std::vector<NbrItem> narrow, wide;
    std::vector<NbrSplit> split;
    int64_t slots = 0;                 // partial slots of all split pairs
    int64_t longest = 0;               // elements of the longest item
    int64_t empty = 0;                 // pairs with la == 0: no item
};

// The first pair with an id outside [0, n) (*self_pair = false) or with st == ed (*self_pair = true), or -1.
int64_t nbr_first_bad_pair(int64_t n, int64_t m, const int32_t *st, const int32_t *ed, bool *self_pair);

// Both orientations of every arc, self-loops dropped, repeats merged: row_ptr [n + 1], col (each row ascending, duplicate-free), deg [n].
// Counting sort by row, then sort and dedupe per row.  Inputs already checked.
void nbr_build_graph(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, std::vector<int64_t> &row_ptr, std::vector<int32_t> &col,
                     std::vector<int32_t> &deg);
// which 0: w[i] = 1.0 / std::log((double)deg[i]) for deg >= 2; which 1: w[i] = 1.0 / (double)deg[i] for deg >= 1; otherwise 0.
void nbr_weights(int64_t n, const int32_t *deg, int which, double *w);
// The work items of m checked pairs; a function of deg and the pairs alone.  false when the partial slots would reach 2^31.
bool nbr_plan(const int32_t *deg, int64_t m, const int32_t *st, const int32_t *ed, NbrPlan &plan);

}  // namespace gemhip
