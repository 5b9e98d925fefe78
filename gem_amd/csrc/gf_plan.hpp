// gf_plan.hpp -- the host arithmetic of Graph Factorization (gf_plan.hip): which edge orders two table copies can represent, the row plan (first-visit
// order, levels, hub rows first), the unit plan of any edge order, the launches of a unit sweep, the rows-per-wavefront rule.  Plain C++, no HIP:
// everything here runs on a CPU (scripts/build_asan_gf_plan.sh, tests/test_gf_plan.py), gf.hip only words the refusals, uploads and launches.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gemhip {

// What a planner found wrong with an edge list.  The planners never word a message: the C ABI around them (gf.hip) does.
struct GfPlanError {
    enum Kind { NONE = 0, EDGE_OUT_OF_RANGE, PARTLY_UPDATED, TOO_MANY_UNITS } kind = NONE;
    int64_t edge = -1;                 // the first offending edge (EDGE_OUT_OF_RANGE, PARTLY_UPDATED)
    int64_t first = -1, last = -1;     // PARTLY_UPDATED: the firing edges of the row that edge reads span these positions
    explicit operator bool() const { return kind != NONE; }
};

struct GfSeg { int l0, l1; bool fused; };   // one launch of a unit sweep: [l0, l1) is one level, or a fused run of small levels

// One plan, as the kernels read it.  Row plan: rows = row ids in processing order (sorted by level; inside a level hub rows first, the others in the
// reference's visiting order), ptr = CSR offsets over rows, col = neighbour id | (1u << 31 if that neighbour is read from X_new).  Unit plan (units):
// the same arrays read differently -- rows holds one entry per UNIT (a run of one row's edges), row id | (1u << 31 if the unit loads its own row from
// X_new), ptr / col / w its edges in file order, level_off the units of each level, segs the launches of a sweep; level_hubs / level_maxlen stay empty.
struct GfHostPlan {
    bool units = false;
    int64_t nrows = 0, nupd = 0;       // rows (units), firing edges
    std::vector<int32_t> rows;
    std::vector<int64_t> ptr;
    std::vector<uint32_t> col;
    std::vector<float> w;
    std::vector<int64_t> level_off;    // rows of level L are [level_off[L], level_off[L+1])
    std::vector<int64_t> level_hubs;   // ... of which the first level_hubs[L] are hub rows
    std::vector<int64_t> level_maxlen; // longest non-hub row of the level, in firing edges
    std::vector<GfSeg> segs;
};

// Can the row plan (one wavefront per source row, two table copies) reproduce the sequential loop over this edge order (the rule: gf_plan.hip)?
// Returns the first edge with an endpoint outside [0, n), else the first edge that reads a partly updated row, else NONE.
// gem_amd/graph.py:row_schedule_represents restates the second part on numpy arrays.
GfPlanError gf_check_row_order(int64_t n, int64_t m, const int32_t *src, const int32_t *dst);

// The row plan of the source rows in [row_begin, row_end).  hub_edges > 0: rows with at least that many firing edges come first in their level.
// On an error P is left as it was.
GfPlanError gf_plan_rows(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int64_t row_begin, int64_t row_end,
                         int64_t hub_edges, GfHostPlan &P);

// The any-order rule (gf_plan.hip), per edge and per unit in creation order.
struct GfUnitSchedule {
    std::vector<int32_t> unit_of;         // per edge: its unit (creation order), -1 = does not fire
    std::vector<uint8_t> nb_new;          // per edge: the neighbour is read from X_new
    std::vector<int32_t> row, level;      // per unit
    std::vector<uint8_t> own_new;         // per unit: its own row is loaded from X_new
    int32_t nlevels = 0;
    int64_t nupd = 0;
};
GfPlanError gf_schedule_units(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, GfUnitSchedule &S);

// The unit plan: units sorted by level (inside a level: creation order), each unit's edges in file order, segs for `fused_levels`.
GfPlanError gf_plan_units(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int fused_levels, GfHostPlan &P);

// the launches of one sweep of a unit plan; fused_levels 0 = never fuse
std::vector<GfSeg> gf_units_segments(const std::vector<int64_t> &level_off, int fused_levels);

// rows per wavefront of the sweep launch over `nrows` rows of a level whose longest non-hub row has `maxlen` firing edges; forced > 0 overrides
int gf_level_rows_per_wave(int forced, int64_t maxlen, int64_t nrows, int kmax);

// ---- blocked hub rows (gf_hub_block_kernel, gemhip_gf_plan_set_hub_block): B edges of a hub row are applied with one Gram matrix of their neighbour
// rows, B scalar steps and one GEMV instead of B dependent dot-and-axpy steps.
constexpr int GF_HUB_BLOCK_MAX = 32;
// floats of a row as the kernels stage it: a lane holds 2 floats (even d) or 1 (odd d) of each of 1, 2, 4 or 8 64-lane chunks; 0 = d unsupported
int gf_row_floats(int d);
// B for a staged row of `row_floats` floats: one 32x32 fp32 MFMA tile while B rows, their Gram matrix and a ring of such stages fit a CU's LDS,
// one 16x16 tile for the wide rows
constexpr int gf_hub_block_of_row_floats(int row_floats) { return row_floats <= 256 ? 32 : 16; }
// B for width d (0 = d unsupported)
int gf_hub_block(int d);
// hi[k] = fl32(a^k), lo[k] = fl32(a^k - hi[k]) for k = 0..B, a = 1 - (double)eta * (double)regu and its powers evaluated in double: the decay a block
// applies to the row and to the earlier steps of the block.  (Repeated fp32 multiplication by fl32(a) carries fl32(a)'s representation error into
// every step, systematically: DESIGN.md "GF: blocked hub rows".)
void gf_hub_decay(float eta, float regu, int B, float *hi, float *lo);

}  // namespace gemhip
