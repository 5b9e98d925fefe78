// gf_plan.hip -- the host arithmetic of Graph Factorization on gfx950: the acceptance rule of the row plan, the row plan, the any-order unit schedule and
// its plan, the launches of a unit sweep, the rows-per-wavefront rule.  HIP-free by rule: no HIP header, nothing from common.hpp -- the `.hip` suffix
// only serves the build's csrc/*.hip glob, and the file is also valid `clang++ -x c++ -std=c++17` input (scripts/build_asan_gf_plan.sh runs it under
// AddressSanitizer / UBSan with a driver of its own, tests/test_gf_plan.py compares that driver's output with tests/golden/gf_plan_digest.txt and the
// row plans with a numpy restatement).  gf.hip holds the C ABI around it.
#include "gf_plan.hpp"

namespace gemhip {

// The row plan gives a source row ONE wavefront and all of its firing edges in one go, reading X_new[j] for neighbours whose row comes earlier in
// first-visit order and X_old[j] otherwise.  That equals the reference's strictly sequential loop (gf.py:93-100, gf.cpp:152-164) iff every firing
// edge (i,j) at position t sees either ALL of j's updates of this sweep (j's last firing edge is before t, and j was first visited before i) or NONE
// (j's first firing edge is after t) -- always true when a source's edges are contiguous (graph.edges(), saveGraphToEdgeListTxt), and for many
// interleaved lists too.  A list that needs an intermediate version of a row (e.g. (1,2),(0,1),(1,3): row 0 must see X_1 between its two updates)
// has no schedule with two table versions.
GfPlanError gf_check_row_order(int64_t n, int64_t m, const int32_t *src, const int32_t *dst)
{
    GfPlanError err;
    std::vector<int64_t> first_t(n, -1), last_t(n, -1);
    for (int64_t e = 0; e < m; ++e) {
        const int32_t i = src[e], j = dst[e];
        if (i < 0 || i >= n || j < 0 || j >= n) { err.kind = GfPlanError::EDGE_OUT_OF_RANGE; err.edge = e; return err; }
        if (j <= i) continue;                        // does not fire (gf.py:95, gf.cpp:157)
        if (first_t[i] < 0) first_t[i] = e;
        last_t[i] = e;
    }
    for (int64_t e = 0; e < m; ++e) {
        const int32_t i = src[e], j = dst[e];
        if (j <= i || first_t[j] < 0) continue;      // j never fires: its row is the same in both tables
        if (!(first_t[j] < first_t[i] ? last_t[j] < e : first_t[j] > e)) {
            err.kind = GfPlanError::PARTLY_UPDATED; err.edge = e; err.first = first_t[j]; err.last = last_t[j];
            return err;
        }
    }
    return err;
}

GfPlanError gf_plan_rows(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int64_t row_begin, int64_t row_end,
                         int64_t hub_edges, GfHostPlan &P)
{
    if (const GfPlanError err = gf_check_row_order(n, m, src, dst)) return err;       // rejected instead of silently reordered
    // 1. rows in the order the reference first visits them; keep only firing edges (dst > src) of owned rows.
    std::vector<int32_t> pos(n, -1);          // pos[i] = rank of row i among firing source rows (reference order)
    std::vector<int32_t> order;               // row ids by pos
    std::vector<int64_t> deg;
    for (int64_t e = 0; e < m; ++e) {
        const int32_t i = src[e], j = dst[e];
        if (j <= i || i < row_begin || i >= row_end) continue;
        if (pos[i] < 0) { pos[i] = (int32_t)order.size(); order.push_back(i); deg.push_back(0); }
        ++deg[pos[i]];
    }
    const int64_t nrows = (int64_t)order.size();
    std::vector<int64_t> off(nrows + 1, 0);
    for (int64_t r = 0; r < nrows; ++r) off[r + 1] = off[r] + deg[r];
    const int64_t nupd = off[nrows];
    std::vector<uint32_t> col(nupd);
    std::vector<float> wt(nupd);
    {
        std::vector<int64_t> fill(off.begin(), off.end() - 1);
        for (int64_t e = 0; e < m; ++e) {
            const int32_t i = src[e], j = dst[e];
            if (j <= i || i < row_begin || i >= row_end) continue;
            const int64_t q = fill[pos[i]]++;
            col[q] = (uint32_t)j;
            wt[q] = w ? w[e] : 1.0f;
        }
    }
    // 2. levels: row i must run after every neighbour j (j>i) that the reference visits earlier.
    std::vector<int32_t> level(nrows, 0);
    int32_t nlevels = nrows ? 1 : 0;
    for (int64_t r = 0; r < nrows; ++r) {
        int32_t lv = 0;
        for (int64_t q = off[r]; q < off[r + 1]; ++q) {
            const int32_t pj = pos[col[q]];
            if (pj >= 0 && pj < r) {          // j already updated in this sweep -> read X_new[j]
                col[q] |= 0x80000000u;
                lv = std::max(lv, level[pj] + 1);
            }
        }
        level[r] = lv;
        nlevels = std::max(nlevels, lv + 1);
    }
    // 3. stable sort rows by level
    std::vector<int64_t> lvl_cnt(nlevels + 1, 0);
    for (int64_t r = 0; r < nrows; ++r) ++lvl_cnt[level[r] + 1];
    for (int32_t l = 0; l < nlevels; ++l) lvl_cnt[l + 1] += lvl_cnt[l];
    std::vector<int64_t> level_hubs;
    std::vector<int32_t> rows_sorted(nrows);
    std::vector<int64_t> ptr_sorted(nrows + 1, 0);
    std::vector<uint32_t> col_sorted(nupd);
    std::vector<float> w_sorted(nupd);
    {
        // inside a level the rows are independent: hub rows (gf_hub_kernel) first, the others keep the reference's visiting order
        std::vector<int64_t> at(lvl_cnt.begin(), lvl_cnt.end() - 1);
        std::vector<int64_t> newpos(nrows);
        level_hubs.assign(nlevels, 0);
        auto hub = [&](int64_t r) { return hub_edges > 0 && off[r + 1] - off[r] >= hub_edges; };
        for (int64_t r = 0; r < nrows; ++r) if (hub(r)) { newpos[r] = at[level[r]]++; ++level_hubs[level[r]]; }
        for (int64_t r = 0; r < nrows; ++r) if (!hub(r)) newpos[r] = at[level[r]]++;
        std::vector<int64_t> inv(nrows);
        for (int64_t r = 0; r < nrows; ++r) inv[newpos[r]] = r;
        for (int64_t s = 0; s < nrows; ++s) {
            const int64_t r = inv[s];
            rows_sorted[s] = order[r];
            ptr_sorted[s + 1] = ptr_sorted[s] + (off[r + 1] - off[r]);
            std::copy(col.begin() + off[r], col.begin() + off[r + 1], col_sorted.begin() + ptr_sorted[s]);
            std::copy(wt.begin() + off[r], wt.begin() + off[r + 1], w_sorted.begin() + ptr_sorted[s]);
        }
    }

    P = GfHostPlan();
    P.nrows = nrows; P.nupd = nupd;
    P.level_off.assign(lvl_cnt.begin(), lvl_cnt.end());
    P.level_hubs = level_hubs;
    P.level_maxlen.assign(nlevels, 0);
    for (int32_t l = 0; l < nlevels; ++l)
        for (int64_t q = lvl_cnt[l] + level_hubs[l]; q < lvl_cnt[l + 1]; ++q) P.level_maxlen[l] = std::max(P.level_maxlen[l], ptr_sorted[q + 1] - ptr_sorted[q]);
    P.rows.swap(rows_sorted); P.ptr.swap(ptr_sorted); P.col.swap(col_sorted); P.w.swap(w_sorted);
    return GfPlanError();
}

// The any-order rule.  Walk the firing edges in file order; per row r: lastW[r] = level of the last unit that wrote r in this sweep (-1: not written
// yet, the row is read from X_old), lastR[r] = highest level of a read of the CURRENT X_new version of r (-1 after every write of r; reads of X_old
// never count: X_old is not written during the sweep), lastU[r] = r's latest unit.  Edge (i, j) must run after j's last write when it reads X_new[j]
// (read after write) and after every read of i's current intermediate version (write after read): c is the higher of the two.  It joins i's latest
// unit when that unit already runs after c, else it opens a unit one level above c and above i's last write.  Two firing edges that touch a common row
// which one of them writes therefore sit in strictly ordered levels, or in one unit in file order: the result equals the sequential loop.  O(n + m).
GfPlanError gf_schedule_units(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, GfUnitSchedule &S)
{
    GfPlanError err;
    std::vector<int32_t> lastW(n, -1), lastR(n, -1), lastU(n, -1);
    S.unit_of.assign(m, -1); S.nb_new.assign(m, 0);
    for (int64_t e = 0; e < m; ++e) {
        const int32_t i = src[e], j = dst[e];
        if (!(i >= 0 && i < n && j >= 0 && j < n)) { err.kind = GfPlanError::EDGE_OUT_OF_RANGE; err.edge = e; return err; }
        if (j <= i) continue;                        // does not fire (gf.py:95, gf.cpp:157)
        if (!(S.row.size() < (size_t)0x7fffffff)) { err.kind = GfPlanError::TOO_MANY_UNITS; err.edge = e; return err; }
        const bool jn = lastW[j] >= 0;
        const int32_t c = std::max(lastW[j], lastR[i]);
        int32_t lv, u;
        if (lastW[i] >= 0 && c < lastW[i]) { u = lastU[i]; lv = lastW[i]; }
        else {
            lv = std::max(c, lastW[i]) + 1;
            u = (int32_t)S.row.size();
            S.row.push_back(i); S.level.push_back(lv); S.own_new.push_back(lastW[i] >= 0);
            lastU[i] = u;
            S.nlevels = std::max(S.nlevels, lv + 1);
        }
        S.unit_of[e] = u; S.nb_new[e] = jn; ++S.nupd;
        if (jn) lastR[j] = std::max(lastR[j], lv);
        lastW[i] = lv; lastR[i] = -1;
    }
    return err;
}

GfPlanError gf_plan_units(int64_t n, int64_t m, const int32_t *src, const int32_t *dst, const float *w, int fused_levels, GfHostPlan &P)
{
    GfUnitSchedule S;
    if (const GfPlanError err = gf_schedule_units(n, m, src, dst, S)) return err;
    // units sorted by level (inside a level: creation order), each unit's edges in file order
    const int64_t nunits = (int64_t)S.row.size();
    std::vector<int64_t> level_off(S.nlevels + 1, 0);
    for (int64_t u = 0; u < nunits; ++u) ++level_off[S.level[u] + 1];
    for (int32_t l = 0; l < S.nlevels; ++l) level_off[l + 1] += level_off[l];
    std::vector<int64_t> slot(nunits), ptr(nunits + 1, 0);
    std::vector<int32_t> units(nunits);
    {
        std::vector<int64_t> at(level_off.begin(), level_off.end() - 1);
        for (int64_t u = 0; u < nunits; ++u) {
            slot[u] = at[S.level[u]]++;
            units[slot[u]] = (int32_t)((uint32_t)S.row[u] | (S.own_new[u] ? 0x80000000u : 0u));
        }
    }
    for (int64_t e = 0; e < m; ++e) if (S.unit_of[e] >= 0) ++ptr[slot[S.unit_of[e]] + 1];
    for (int64_t u = 0; u < nunits; ++u) ptr[u + 1] += ptr[u];
    std::vector<uint32_t> col(S.nupd);
    std::vector<float> wt(S.nupd);
    {
        std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
        for (int64_t e = 0; e < m; ++e) {
            if (S.unit_of[e] < 0) continue;
            const int64_t q = fill[slot[S.unit_of[e]]]++;
            col[q] = (uint32_t)dst[e] | (S.nb_new[e] ? 0x80000000u : 0u);
            wt[q] = w ? w[e] : 1.0f;
        }
    }
    P = GfHostPlan();
    P.units = true; P.nrows = nunits; P.nupd = S.nupd;
    P.segs = gf_units_segments(level_off, fused_levels);
    P.rows.swap(units); P.ptr.swap(ptr); P.col.swap(col); P.w.swap(wt); P.level_off.swap(level_off);
    return GfPlanError();
}

// every maximal run of two or more consecutive levels of at most fused_levels units is one launch (gf_units_fused_kernel), every other level one
// (gf_sweep_units_kernel)
std::vector<GfSeg> gf_units_segments(const std::vector<int64_t> &level_off, int fused_levels)
{
    std::vector<GfSeg> segs;
    const int nlevels = (int)level_off.size() - 1;
    auto small = [&](int l) { return fused_levels > 0 && level_off[l + 1] - level_off[l] <= fused_levels; };
    for (int l = 0; l < nlevels;) {
        int e = l + 1;
        if (small(l)) while (e < nlevels && small(e)) ++e;
        segs.push_back({l, e, e - l > 1});
        l = e;
    }
    return segs;
}

// 1 row per wavefront (gf_sweep_kernel) until every resident wave slot of the chip (256 CUs x 32 waves) has two rows to work on, then up to kmax
// (gf_sweep_rows_kernel): a level of 946 188 rows (SBM 1M/10M) runs 8 rows per wave at kmax = 8.
// K rows per wavefront pays where rows are short and alike (SBM: 548 against 579 us per sweep at 1M/10M); on a power-law level a wavefront that
// draws a few long rows among its K holds the launch up (R-MAT scale 22: 6.99 against 6.52 ms) -- levels with rows of more than two 64-edge
// chunks keep one row per wavefront
int gf_level_rows_per_wave(int forced, int64_t maxlen, int64_t nrows, int kmax)
{
    if (forced > 0) return forced;
    if (maxlen > 2 * 64) return 1;
    return (int)std::max<int64_t>(1, std::min<int64_t>(nrows / (2 * 256 * 32), kmax));
}

int gf_row_floats(int d)
{
    if (d < 1) return 0;
    const int vec = d % 2 == 0 ? 2 : 1, chunks = (d + vec * 64 - 1) / (vec * 64);
    const int nv = chunks <= 1 ? 1 : chunks <= 2 ? 2 : chunks <= 4 ? 4 : chunks <= 8 ? 8 : 0;
    return nv * vec * 64;
}

int gf_hub_block(int d)
{
    const int rw = gf_row_floats(d);
    return rw ? gf_hub_block_of_row_floats(rw) : 0;
}

void gf_hub_decay(float eta, float regu, int B, float *hi, float *lo)
{
    const double a = 1.0 - (double)eta * (double)regu;
    double p = 1.0;                                   // a^k by repeated DOUBLE multiplication: k <= 32 roundings of 2^-53 each
    for (int k = 0; k <= B; ++k) {
        hi[k] = (float)p;
        lo[k] = (float)(p - (double)hi[k]);
        p *= a;
    }
}

}  // namespace gemhip
