// Stand-alone driver of gem_amd/csrc/hope_host.hip (the host arithmetic of HOPE / Laplacian Eigenmaps / LLE): plain C++, no HIP, no device.  Links
// hope_host.hip and sym_eig.hip.
//
//   hope_host_driver <group> <in> <out>      group: dense | ritz | sym | krylov | out | csr
//       Both files are a sequence of fp64 arrays, each preceded by its length as one fp64 (integers travel as fp64 too).  The arrays of every
//       group are listed at its function below; tests/test_hope_host.py writes the inputs and compares the outputs with numpy.
//   hope_host_driver knobs <out> [NAME=VALUE ...]
//       hope_knobs_from_env over exactly the variables given (a table, never the process's environment): one array, listed at run_knobs below.
//   hope_host_driver self
//       every function on inputs generated from seeds, the awkward ones included (a null Gram column, a repeated column, keep = 2, no column to
//       lock, want = 1, tau = 0, tau >= 1, every kind, an empty row, nnz = 0, one differing weight, duplicate entries), the knobs (defaults, each
//       variable alone, the clamps, present-but-empty) and check_csr_arrays against the test hooks' rule; checks C^T G C = I and the
//       like, prints one line per check, returns 1 if one failed.  scripts/build_asan_hope_host.sh runs this form under AddressSanitizer and UBSan.
#include "../../gem_amd/csrc/hope_host.hpp"
#include "../../gem_amd/csrc/sym_eig.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

using namespace gemhip;

namespace {

typedef std::vector<double> Vec;

bool read_arrays(const char *path, std::vector<Vec> &A)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    double len;
    while (fread(&len, 8, 1, f) == 1) {
        Vec v((size_t)len);
        if (fread(v.data(), 8, v.size(), f) != v.size()) { fclose(f); return false; }
        A.push_back(v);
    }
    fclose(f);
    return true;
}

bool write_arrays(const char *path, const std::vector<Vec> &A)
{
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    for (const Vec &v : A) { const double len = (double)v.size(); fwrite(&len, 8, 1, f); fwrite(v.data(), 8, v.size(), f); }
    return fclose(f) == 0;
}

// in: {b, tol, abs_floor}, G (b x b), H (b x b)
// out: {nk, remixed}, C of orth_pass; {nk}, C of orth_scaled_pass; {ok}, C2, Hq of rr_project; dinv, normalised G; {ok}, C of chol_inverse(floor 0)
std::vector<Vec> run_dense(const std::vector<Vec> &in)
{
    const int b = (int)in[0][0];
    Vec G = in[1], C;
    bool remixed = false;
    const int nk = orth_pass(b, G, in[0][1], in[0][2], C, &remixed);
    std::vector<Vec> out = {{(double)nk, (double)remixed}, nk ? C : Vec()};
    G = in[1]; C.clear();
    const int ns = orth_scaled_pass(b, G, C);
    out.push_back({(double)ns}); out.push_back(ns ? C : Vec());
    G = in[1];
    Vec H = in[2], C2;
    const bool ok = rr_project(b, G, H, C2);
    out.push_back({(double)ok}); out.push_back(C2); out.push_back(H);
    G = in[1];
    out.push_back(normalise_gram(b, G)); out.push_back(G);
    C.clear();
    const bool cok = chol_inverse(b, in[1], 0.0, C);
    out.push_back({(double)cok}); out.push_back(cok ? C : Vec());
    return out;
}

// in: {ma, kind, beta}, Z (ma x ma, eigenvectors in columns), ev (ascending), C2 (ma x ma or empty), M (ma x ma)      out: th, C, Ct, sym(M), f(ev)
std::vector<Vec> run_ritz(const std::vector<Vec> &in)
{
    const int ma = (int)in[0][0], kind = (int)in[0][1];
    Vec th, C, Ct, M = in[4], f;
    ritz_order(ma, in[1], in[2], kind, in[0][2], in[3], th, C, Ct);
    symmetrise(ma, M);
    for (double x : in[2]) f.push_back(sym_f(kind, in[0][2], x));
    return {th, C, Ct, M, f};
}

// in: {kind, beta, br, lo, hi, nl, cyc, amp, amp0, max_degree, want, b_min, tol, tau_prev}, th, res
// out: {L, smin, smax, res_floor, lo0, hi0}, {c, e, q, m}, {rmax, newl}, {jc, tau_prev, lo, hi} (as the solver: after the newl leading pairs left th)
std::vector<Vec> run_sym(const std::vector<Vec> &in)
{
    const Vec &a = in[0];
    const int kind = (int)a[0], nl = (int)a[5], want = (int)a[10];
    const SymSpectrum sp = sym_spectrum(kind, a[1], a[2]);
    double lo0, hi0, lo = a[3], hi = a[4], tau_prev = a[13];
    sym_first_interval(kind, sp.L, lo0, hi0);
    const SymCycle cy = sym_cycle_plan(lo, hi, sp.smin, sp.smax, in[1], nl, (int)a[6], a[7], a[8], (int)a[9]);
    const double rmax = sym_residual_scale(want, in[1], in[2], sp.L, sp.res_floor);
    const int newl = sym_lock_count(want, (int)a[11], in[1], in[2], lock_tolerance((float)a[12]), sp.res_floor);
    const Vec th(in[1].begin() + newl, in[1].end());
    const int jc = th.empty() ? -1 : sym_next_interval(kind, a[1], sp.L, want - newl, th, tau_prev, lo, hi);
    return {{sp.L, sp.smin, sp.smax, sp.res_floor, lo0, hi0}, {cy.c, cy.e, (double)cy.q, (double)cy.m}, {rmax, (double)newl}, {(double)jc, tau_prev, lo, hi}};
}

// in: {b, krylov_steps, n, has_basis, basis, nl, m0, has_depth, depth, oversample, tol, want, prev_b, mt, ma}, act_sig, D (prev_b x prev_b), Zt (ma x mt column-major)
// out: {mmax, steps, b_min, lock_tol, newl, nb}, C (ma x nb)
std::vector<Vec> run_krylov(const std::vector<Vec> &in)
{
    const Vec &a = in[0];
    const int b = (int)a[0], basis = (int)a[4], nl = (int)a[5], depth = (int)a[8];
    const int mmax = krylov_basis_capacity(b, (int)a[1], (int64_t)a[2], a[3] != 0.0 ? &basis : nullptr);
    const int steps = krylov_steps_after_lock((int)a[1], mmax, nl, (int)a[6], a[7] != 0.0 ? &depth : nullptr);
    const int b_min = krylov_b_min(b, (int)a[9]);
    const double lock_tol = lock_tolerance((float)a[10]);
    const int newl = krylov_lock_count((int)a[11], (int)a[12], b_min, in[1], in[2], lock_tol);
    Vec C;
    const int nb = krylov_restart_block((int)a[13], b, nl, b_min, (int)a[14], in[3], C);
    return {{(double)mmax, (double)steps, (double)b_min, lock_tol, (double)newl, (double)nb}, C};
}

// in: {k, nl, ma, has_Zt, from_image, unit_v}, all, sig_old, cand (s, sgn, col per candidate), Zt, colmax (k)
// out: sig, {change}, sig_old, sigma, Cu, Cv, {any}, flipped Cu, flipped Cv, order (the candidates' columns after the sort), stats (12)
std::vector<Vec> run_out(const std::vector<Vec> &in)
{
    const Vec &a = in[0];
    const int k = (int)a[0], nl = (int)a[1], ma = (int)a[2];
    Vec sig(k, 0.0), sig_old = in[2], Cu, Cv, order;
    const double change = wanted_values(in[1], k, sig, sig_old);
    std::vector<OutCand> cand;
    for (size_t i = 0; i + 2 < in[3].size(); i += 3) cand.push_back({in[3][i], in[3][i + 1], (int)in[3][i + 2]});
    std::vector<float> sigma(k, 0.f);
    select_outputs(cand, k, nl, ma, a[3] != 0.0 ? &in[4] : nullptr, a[4] != 0.0, a[5] != 0.0, sigma.data(), Cu, Cv);
    for (const OutCand &c : cand) order.push_back(c.col);
    Vec Fu = Cu, Fv = Cv, stats(12, 0.0);
    const bool any = flip_negative_columns(nl + ma, k, in[5], Fu, Fv);
    reset_eig_stats();
    fill_solve_stats(stats.data(), 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0, 10.0);
    return {sig, {change}, sig_old, Vec(sigma.begin(), sigma.end()), Cu, Cv, {(double)any}, Fu, Fv, order, stats};
}

// in: {n, nnz, has_w, br, k}, row_ptr, col, w        out: {error, bad_edge}; if error == 0: rpT, ciT, vaT, {symmetric, bound, terms}, Laplacian-Eigenmaps
// values, LLE values, w (padded to a multiple of k) as rows of k with the columns reversed
std::vector<Vec> run_csr(const std::vector<Vec> &in)
{
    const int64_t n = (int64_t)in[0][0], nnz = (int64_t)in[0][1];
    const int k = (int)in[0][4];
    const std::vector<int64_t> rp(in[1].begin(), in[1].end());
    const std::vector<int32_t> ci(in[2].begin(), in[2].end());
    std::vector<float> w(in[3].begin(), in[3].end());
    w.resize(std::max<size_t>(std::max<int64_t>(nnz, 1), w.size()), 1.0f);
    int64_t bad = -1;
    const CsrError err = check_csr_arrays(n, nnz, rp.data(), ci.data(), &bad);
    std::vector<Vec> out = {{(double)(int)err, (double)bad}};
    if (err != CsrError::NONE) return out;
    const CsrT T = transpose_csr(n, nnz, rp.data(), ci.data(), w.data());
    out.push_back(Vec(T.rp.begin(), T.rp.end())); out.push_back(Vec(T.ci.begin(), T.ci.begin() + nnz)); out.push_back(Vec(T.va.begin(), T.va.begin() + nnz));
    out.push_back({(double)csr_is_symmetric(n, nnz, rp.data(), T), abs_sum_bound(n, rp.data(), ci.data(), w.data()), (double)katz_terms(in[0][3])});
    std::vector<float> va(std::max<int64_t>(nnz, 1));
    const float *wp = in[0][2] != 0.0 ? w.data() : nullptr;
    lap_edge_values(n, rp.data(), ci.data(), wp, va.data());
    out.push_back(Vec(va.begin(), va.begin() + nnz));
    lle_edge_values(n, rp.data(), wp, va.data());
    out.push_back(Vec(va.begin(), va.begin() + nnz));
    std::vector<float> R(w.begin(), w.end());
    R.resize((R.size() + k - 1) / k * k, 0.f);
    reverse_columns(R.data(), (int64_t)(R.size() / k), k);
    out.push_back(Vec(R.begin(), R.end()));
    return out;
}

// The environment hope_knobs_from_env is shown: NAME=VALUE strings, never the process's own
std::vector<std::string> fake_env;
const char *fake_lookup(const char *name)
{
    const size_t len = strlen(name);
    for (const std::string &s : fake_env)
        if (s.size() > len && s.compare(0, len, name) == 0 && s[len] == '=') return s.c_str() + len + 1;
    return nullptr;
}

// out: {spmm16, spmm16_u, colmax2, sym, sym_amp, sym_amp0, sym_maxdeg, sym_fused_rr, no_lock, fixed_depth, host_project, debug, has_basis_cols, basis_cols,
// has_depth_cols, depth_cols} of hope_knobs_from_env over exactly the variables in `env`; the two overrides are read through their accessors
Vec run_knobs(const std::vector<std::string> &env)
{
    fake_env = env;
    const HopeKnobs kn = hope_knobs_from_env(fake_lookup);
    const int *bc = kn.basis_cols_override(), *dc = kn.depth_cols_override();
    return {(double)kn.spmm16, (double)kn.spmm16_u, (double)kn.colmax2, (double)kn.sym, kn.sym_amp, kn.sym_amp0, (double)kn.sym_maxdeg, (double)kn.sym_fused_rr,
            (double)kn.no_lock, (double)kn.fixed_depth, (double)kn.host_project, (double)kn.debug, (double)(bc != nullptr), bc ? (double)*bc : 0.0,
            (double)(dc != nullptr), dc ? (double)*dc : 0.0};
}

// ------------------------------------------------------------------ self
int failures = 0;
void check(const char *what, bool ok) { printf("%-72s %s\n", what, ok ? "ok" : "FAILED"); failures += !ok; }

// only raw mt19937 words are used (no <random> distribution: those differ between standard libraries)
double unit(std::mt19937 &mt) { return ((double)(mt() >> 5) + 0.5) / 134217728.0 - 0.5; }

Vec gram_of(int n, int b, const Vec &Y)
{
    Vec G((size_t)b * b, 0.0);
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < b; ++i)
            for (int j = 0; j < b; ++j) G[(size_t)i * b + j] += Y[(size_t)r * b + i] * Y[(size_t)r * b + j];
    return G;
}

// max |C^T G C - I| over the nk kept columns
double orth_defect(int b, int nk, const Vec &G, const Vec &C)
{
    double worst = 0.0;
    for (int p = 0; p < nk; ++p)
        for (int q = 0; q < nk; ++q) {
            double v = 0.0;
            for (int i = 0; i < b; ++i)
                for (int j = 0; j < b; ++j) v += C[(size_t)i * nk + p] * G[(size_t)i * b + j] * C[(size_t)j * nk + q];
            worst = std::max(worst, std::fabs(v - (p == q ? 1.0 : 0.0)));
        }
    return worst;
}

void self_dense(uint32_t seed)
{
    std::mt19937 mt(seed);
    for (int b : {2, 5, 24}) {
        const int n = 3 * b + 7;
        Vec Y((size_t)n * b), Hm((size_t)b * b);
        for (double &y : Y) y = unit(mt);
        for (double &h : Hm) h = unit(mt);
        for (int r = 0; r < n; ++r) Y[(size_t)r * b + b - 1] *= 20.0;                     // columns of different length
        const Vec G = gram_of(n, b, Y);
        std::vector<Vec> o = run_dense({{(double)b, 1e-10, 0.0}, G, Hm});
        check(("full rank: orth_pass keeps every column, C^T G C = I, b=" + std::to_string(b)).c_str(), o[0][0] == b && o[0][1] == 0.0 && orth_defect(b, b, G, o[1]) < 1e-9);
        check("full rank: orth_scaled_pass keeps every column, C^T G C = I", o[2][0] == b && orth_defect(b, b, G, o[3]) < 1e-9);
        check("full rank: rr_project succeeds, C2^T G C2 = I", o[4][0] == 1.0 && orth_defect(b, b, G, o[5]) < 1e-9);
        Vec Yr = Y;                                                                        // exactly rank deficient: the last column repeats the first
        for (int r = 0; r < n; ++r) Yr[(size_t)r * b + b - 1] = Yr[(size_t)r * b];
        const Vec Gr = gram_of(n, b, Yr);
        o = run_dense({{(double)b, 1e-10, 0.0}, Gr, Hm});
        check("repeated column: orth_pass takes the fallback and drops one direction", o[0][0] == b - 1 && o[0][1] == 1.0 && orth_defect(b, b - 1, Gr, o[1]) < 1e-9);
        check("repeated column: orth_scaled_pass drops one direction", o[2][0] == b - 1 && orth_defect(b, b - 1, Gr, o[3]) < 1e-6);
        check("repeated column: rr_project refuses and leaves H alone", o[4][0] == 0.0 && o[5].empty() && o[6] == Hm);
        Vec Yz = Y;                                                                        // a null column: zero diagonal entry
        for (int r = 0; r < n; ++r) Yz[(size_t)r * b + 1] = 0.0;
        const Vec Gz = gram_of(n, b, Yz);
        o = run_dense({{(double)b, 1e-10, 0.0}, Gz, Hm});
        check("null column: dinv is 0 there, orth_scaled_pass drops it, rr_project refuses", o[7][1] == 0.0 && o[2][0] == b - 1 && o[4][0] == 0.0 && orth_defect(b, b - 1, Gz, o[3]) < 1e-9);
        o = run_dense({{(double)b, 1e-10, 0.0}, Vec((size_t)b * b, 0.0), Hm});
        check("zero Gram matrix: nothing is kept", o[0][0] == 0.0 && o[2][0] == 0.0 && o[4][0] == 0.0);
        // Ritz ordering of a random symmetric matrix, every kind, with and without C2
        Vec Z = Hm, ev;
        symmetrise(b, Z);
        sym_eig(b, Z, ev);
        for (int kind = 0; kind < 3; ++kind)
            for (int with_c2 = 0; with_c2 < 2; ++with_c2) {
                const double beta = kind == 2 ? 1.5 : 0.3;
                std::vector<Vec> r = run_ritz({{(double)b, (double)kind, beta}, Z, ev, with_c2 ? o[5].empty() ? run_dense({{(double)b, 1e-10, 0.0}, G, Hm})[5] : o[5] : Vec(), Hm});
                bool sorted = true;
                for (int j = 1; j < b; ++j) sorted = sorted && std::fabs(sym_f(kind, beta, r[0][j - 1])) >= std::fabs(sym_f(kind, beta, r[0][j]));
                check(("ritz_order: |f(theta)| descending, kind " + std::to_string(kind)).c_str(), sorted && r[1].size() == (size_t)b * b && r[2].size() == (size_t)b * b);
            }
    }
}

void self_rules()
{
    for (int kind = 0; kind < 3; ++kind) {
        const double beta = kind == 2 ? 1.7 : kind == 1 ? 1.0 : 0.05, br = 0.6;
        const SymSpectrum sp = sym_spectrum(kind, beta, br);
        double lo, hi;
        sym_first_interval(kind, sp.L, lo, hi);
        Vec th = {0.9 * sp.L, -0.8 * sp.L, 0.7 * sp.L, 0.5 * sp.L, 0.4 * sp.L, 0.1 * sp.L}, res = {1e-9, 1e-9, 1e-3, 1e-2, 1e-1, 1e-1};
        if (kind == 2) for (double &t : th) t = std::fabs(sp.L - std::fabs(t));
        for (int cyc : {0, 1, 5})
            for (int nl : {0, 3}) {
                std::vector<Vec> o = run_sym({{(double)kind, beta, br, lo, hi, (double)nl, (double)cyc, 1e4, 1e3, 32, 4, 2, 1e-5, 0.0}, th, res});
                check(("sym rules: 1 <= q, 2 <= m <= 32, lo < hi, kind " + std::to_string(kind)).c_str(),
                      o[1][2] >= 1 && o[1][3] >= 2 && o[1][3] <= 32 && o[3][2] < o[3][3] && o[2][1] >= 0 && o[2][1] <= 3 && o[3][0] >= 0);
            }
        std::vector<Vec> o = run_sym({{(double)kind, beta, br, lo, hi, 0, 1, 1e4, 1e3, 32, 1, 2, 1e-5, 0.0}, th, res});
        check("sym rules: want = 1 locks nothing", o[2][1] == 0.0);
        o = run_sym({{(double)kind, beta, br, lo, hi, 0, 1, 1e4, 1e3, 32, 4, 9, 1e-5, 0.0}, th, res});
        check("sym rules: ma - b_min <= 0 locks nothing", o[2][1] == 0.0);
        const double zero = kind == 0 ? 0.0 : kind == 1 ? -1.0 : beta;                    // f(zero) = 0: tau = 0 -> the first interval again
        o = run_sym({{(double)kind, beta, br, 0.1, 0.2, 0, 1, 1e4, 1e3, 32, 1, 1, 1e-5, 0.0}, {zero}, {1.0}});
        check("sym rules: tau = 0 returns the first interval", o[3][1] == 0.0 && o[3][2] == lo && o[3][3] == hi);
        o = run_sym({{(double)kind, beta, br, lo, hi, 0, 1, 1e4, 1e3, 32, 4, 2, 1e-5, 5.0}, th, res});
        check("sym rules: tau >= 1 (tau_prev = 5) keeps a valid interval", o[3][1] == 5.0 && o[3][2] < o[3][3] && std::isfinite(o[3][2]) && std::isfinite(o[3][3]));
    }
    const Vec act = {3.0, 2.0, 1.0, 0.5}, D = {1e-12, 0, 0, 0, 0, 1e-12, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0}, Zt = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    std::vector<Vec> o = run_krylov({{80, 5, 100000, 0, 0, 0, 0, 0, 0, 16, 1e-5, 4, 4, 3, 4}, act, D, Zt});
    check("krylov rules: default capacity 512, prev_b - b_min <= 0 locks nothing", o[0][0] == 512 && o[0][1] == 5 && o[0][4] == 0);
    o = run_krylov({{4, 5, 100000, 1, 7, 2, 2, 1, 1000, 0, 1e-5, 4, 4, 3, 4}, act, D, Zt});
    check("krylov rules: overrides, locking stops at want - 1 / the tolerance", o[0][0] == 24 && o[0][1] == 10 && o[0][4] == 0 && o[0][5] == 3 && o[1].size() == 12);
    o = run_krylov({{2, 5, 100000, 0, 0, 0, 0, 0, 0, 1, 1e-5, 4, 4, 3, 4}, act, D, Zt});
    check("krylov rules: two converged pairs are locked, the block keeps b_min columns", o[0][2] == 2 && o[0][4] == 2);
    o = run_krylov({{2, 5, 100000, 0, 0, 0, 0, 0, 0, 1, 1e-5, 1, 4, 3, 4}, act, D, Zt});
    check("krylov rules: want = 1 locks nothing", o[0][4] == 0);
}

void self_outputs()
{
    const int k = 3, nl = 2, ma = 3;
    const Vec all = {5.0, 1.0, 4.0, 4.0, 0.5}, Zt = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const Vec cand = {5.0, 1.0, 0, 1.0, -1.0, 1, 4.0, 1.0, 2, 4.0, -1.0, 3, 0.5, 1.0, 4};
    for (int has_zt = 0; has_zt < 2; ++has_zt)
        for (int unit_v = 0; unit_v < 2; ++unit_v) {
            std::vector<Vec> o = run_out({{(double)k, (double)nl, (double)ma, (double)has_zt, (double)has_zt, (double)unit_v}, all, {5.0, 4.0, 3.0}, cand, Zt, {1.0, -1.0, 0.0}});
            check("outputs: sigma ascending, ties keep their order, one column flipped", o[0][0] == 5.0 && o[1][0] == 0.2 && o[3][0] == 4.0 && o[3][2] == 5.0 &&
                  o[9][1] == 2.0 && o[9][2] == 3.0 && o[6][0] == 1.0 && o[7][(size_t)2 * k + 1] == -o[4][(size_t)2 * k + 1] && o[10][0] == 1.0 * 1e-3 && o[10][11] == 10.0 * 1e-3);
        }
    std::vector<Vec> o = run_out({{1, 0, 1, 0, 0, 0}, {0.0}, {0.0}, {0.0, 1.0, 0}, Vec(), {0.0}});
    check("outputs: a zero value gives zero columns and change 0", o[1][0] == 0.0 && o[4][0] == 0.0 && o[5][0] == 0.0);
    o = run_out({{1, 0, 1, 1, 1, 0}, {0.0}, {0.0}, {0.0, 1.0, 0}, {1.0}, {0.0}});
    check("outputs: ... from the image too (no division by zero)", o[4][0] == 0.0 && o[5][0] == 0.0);
}

void self_csr()
{
    // 5 nodes: row 2 empty, a duplicate entry (0, 1) twice, structurally symmetric
    const Vec rp = {0, 3, 5, 5, 6, 8}, ci = {1, 1, 4, 0, 0, 4, 0, 3}, w = {2, 3, 1, 2, 3, 7, 1, 7};
    std::vector<Vec> o = run_csr({{5, 8, 1, 0.5, 3}, rp, ci, w});
    check("csr: duplicates and an empty row transpose to the same matrix: symmetric", o[0][0] == 0.0 && o[4][0] == 1.0 && o[1] == rp && o[2] == ci && o[3] == w);
    Vec w2 = w; w2[7] = 7.5;
    o = run_csr({{5, 8, 1, 0.5, 3}, rp, ci, w2});
    check("csr: one differing weight: not symmetric", o[4][0] == 0.0);
    o = run_csr({{5, 0, 0, 0.0, 2}, {0, 0, 0, 0, 0, 0}, Vec(), Vec()});
    check("csr: nnz = 0: not symmetric, bound 0, one term", o[0][0] == 0.0 && o[4][0] == 0.0 && o[4][1] == 0.0 && o[4][2] == 1.0 && o[1] == Vec(6, 0.0));
    o = run_csr({{5, 8, 1, 0.5, 3}, rp, {1, 1, 4, 0, 0, 5, 0, 3}, w});
    check("csr: a column out of range is reported with its position", o[0][0] == (double)(int)CsrError::COLUMN && o[0][1] == 5.0);
    o = run_csr({{5, 7, 1, 0.5, 3}, rp, ci, w});
    check("csr: row_ptr inconsistent with nnz", o[0][0] == (double)(int)CsrError::ROW_PTR);
    o = run_csr({{1, 0, 0, 0.5, 3}, {0, 0}, Vec(), Vec()});
    check("csr: n < 2 is refused", o[0][0] == (double)(int)CsrError::BAD_ARGUMENTS);
    check("katz_terms: 1 at br <= 0, capped at 400", katz_terms(0.0) == 1 && katz_terms(-1.0) == 1 && katz_terms(0.9499) == 359 && katz_terms(0.99) == 400);
    // check_csr_arrays against the rule of the test hooks (hook_csr_ok, hope_hooks.hip: n >= 1, both ends of row_ptr, row_ptr never decreasing, every
    // column in range).  The two agree on five of these inputs and differ on two, which is why the hooks keep their own.
    const int64_t rp3[] = {0, 2, 3, 3}, rp_first[] = {1, 2, 3, 3}, rp_down[] = {0, 3, 2, 3}, rp_zero[] = {0, 0, 0, 0}, rp_one[] = {0, 0};
    const int32_t ci3[] = {1, 2, 0}, ci_neg[] = {1, -1, 0}, ci_n[] = {1, 3, 0};
    int64_t bad = -1;
    check("validators: n = 0 is refused (as by the hooks)", check_csr_arrays(0, 0, rp_one, nullptr, &bad) == CsrError::BAD_ARGUMENTS);
    check("validators: nnz = 0 with col == NULL is accepted (as by the hooks)", check_csr_arrays(3, 0, rp_zero, nullptr, &bad) == CsrError::NONE);
    check("validators: row_ptr[0] != 0 is refused (as by the hooks)", check_csr_arrays(3, 3, rp_first, ci3, &bad) == CsrError::ROW_PTR);
    check("validators: row_ptr[n] != nnz is refused (as by the hooks)", check_csr_arrays(3, 2, rp3, ci3, &bad) == CsrError::ROW_PTR);
    check("validators: col = -1 is refused at its position (as by the hooks)", check_csr_arrays(3, 3, rp3, ci_neg, &bad) == CsrError::COLUMN && bad == 1);
    check("validators: col = n is refused at its position (as by the hooks)", check_csr_arrays(3, 3, rp3, ci_n, &bad) == CsrError::COLUMN && bad == 1);
    check("validators DIFFER: a decreasing row_ptr with consistent ends passes check_csr_arrays (the hooks refuse it)", check_csr_arrays(3, 3, rp_down, ci3, &bad) == CsrError::NONE);
    check("validators DIFFER: n = 1 is refused by check_csr_arrays (the hooks take it)", check_csr_arrays(1, 0, rp_one, nullptr, &bad) == CsrError::BAD_ARGUMENTS);
}

void self_knobs()
{
    const Vec defaults = {1, 0, 1, -1, 1e4, 1e3, 32, 1, 0, 0, 0, 0, 0, 0, 0, 0};
    check("knobs: nothing set gives the defaults", run_knobs({}) == defaults);
    check("knobs: other variables are not looked at", run_knobs({"GEMHIP_HOPE_SPMM16_UX=4", "GEMHIP_SGNS_FRESH=3", "HOPE_SYM=1"}) == defaults);
    // each variable alone: {assignment, index of the value it changes, the value}; everything else stays at its default
    const struct { const char *env; int at; double v; } one[] = {
        {"GEMHIP_HOPE_SPMM16=0", 0, 0}, {"GEMHIP_HOPE_SPMM16_U=2", 1, 2}, {"GEMHIP_HOPE_COLMAX2=0", 2, 0}, {"GEMHIP_HOPE_SYM=0", 3, 0}, {"GEMHIP_HOPE_SYM=1", 3, 1},
        {"GEMHIP_HOPE_SYM=7", 3, 1}, {"GEMHIP_HOPE_SYM=", 3, 0}, {"GEMHIP_HOPE_SYM_AMP=250.5", 4, 250.5}, {"GEMHIP_HOPE_SYM_AMP=3", 4, 10}, {"GEMHIP_HOPE_SYM_AMP0=30", 5, 30},
        {"GEMHIP_HOPE_SYM_AMP0=-1", 5, 10}, {"GEMHIP_HOPE_SYM_MAXDEG=12", 6, 12}, {"GEMHIP_HOPE_SYM_MAXDEG=1", 6, 2}, {"GEMHIP_HOPE_SYM_FUSED_RR=0", 7, 0},
        {"GEMHIP_HOPE_SYM_FUSED_RR=1", 7, 1}, {"GEMHIP_HOPE_NO_LOCK=1", 8, 1}, {"GEMHIP_HOPE_NO_LOCK=", 8, 1}, {"GEMHIP_HOPE_NO_LOCK=0", 8, 1},
        {"GEMHIP_HOPE_FIXED_DEPTH=1", 9, 1}, {"GEMHIP_HOPE_FIXED_DEPTH=", 9, 1}, {"GEMHIP_HOPE_HOST_PROJECT=1", 10, 1}, {"GEMHIP_HOPE_HOST_PROJECT=", 10, 1},
        {"GEMHIP_HOPE_DEBUG=1", 11, 1}, {"GEMHIP_HOPE_DEBUG=", 11, 1}};
    for (const auto &c : one) {
        Vec want = defaults;
        want[c.at] = c.v;
        check((std::string("knobs: ") + c.env).c_str(), run_knobs({c.env}) == want);
    }
    Vec want = defaults;
    want[12] = 1; want[13] = 700;
    check("knobs: GEMHIP_HOPE_BASIS_COLS=700 is passed on", run_knobs({"GEMHIP_HOPE_BASIS_COLS=700"}) == want);
    want[13] = -5;
    check("knobs: GEMHIP_HOPE_BASIS_COLS=-5 is passed on as it is (krylov_basis_capacity clamps)", run_knobs({"GEMHIP_HOPE_BASIS_COLS=-5"}) == want);
    want = defaults;
    want[14] = 1; want[15] = 64;
    check("knobs: GEMHIP_HOPE_DEPTH_COLS=64 is passed on", run_knobs({"GEMHIP_HOPE_DEPTH_COLS=64"}) == want);
    check("knobs: all at once", run_knobs({"GEMHIP_HOPE_SPMM16=0", "GEMHIP_HOPE_SPMM16_U=4", "GEMHIP_HOPE_COLMAX2=0", "GEMHIP_HOPE_SYM=1", "GEMHIP_HOPE_SYM_AMP=100",
                                          "GEMHIP_HOPE_SYM_AMP0=50", "GEMHIP_HOPE_SYM_MAXDEG=8", "GEMHIP_HOPE_SYM_FUSED_RR=0", "GEMHIP_HOPE_NO_LOCK=1",
                                          "GEMHIP_HOPE_FIXED_DEPTH=1", "GEMHIP_HOPE_HOST_PROJECT=1", "GEMHIP_HOPE_DEBUG=1", "GEMHIP_HOPE_BASIS_COLS=96",
                                          "GEMHIP_HOPE_DEPTH_COLS=48"}) == Vec({0, 4, 0, 1, 100, 50, 8, 0, 1, 1, 1, 1, 1, 96, 1, 48}));
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "self")) {
        for (uint32_t seed : {1u, 2u, 3u}) self_dense(seed);
        self_rules(); self_outputs(); self_csr(); self_knobs();
        printf("%d checks failed\n", failures);
        return failures ? 1 : 0;
    }
    if (argc >= 3 && !strcmp(argv[1], "knobs")) return write_arrays(argv[2], {run_knobs(std::vector<std::string>(argv + 3, argv + argc))}) ? 0 : 2;
    if (argc == 4) {
        std::vector<Vec> in, out;
        if (!read_arrays(argv[2], in)) { fprintf(stderr, "hope_host_driver: bad input %s\n", argv[2]); return 2; }
        const std::string g = argv[1];
        const size_t need = g == "dense" ? 3 : g == "ritz" ? 5 : g == "sym" ? 3 : g == "krylov" ? 4 : g == "out" ? 6 : g == "csr" ? 4 : 0;
        if (!need || in.size() != need) { fprintf(stderr, "hope_host_driver: group %s takes %zu arrays (got %zu)\n", argv[1], need, in.size()); return 2; }
        out = g == "dense" ? run_dense(in) : g == "ritz" ? run_ritz(in) : g == "sym" ? run_sym(in) : g == "krylov" ? run_krylov(in) : g == "out" ? run_out(in) : run_csr(in);
        return write_arrays(argv[3], out) ? 0 : 2;
    }
    fprintf(stderr, "usage: %s self | dense|ritz|sym|krylov|out|csr <in> <out> | knobs <out> [NAME=VALUE ...]\n", argv[0]);
    return 2;
}
