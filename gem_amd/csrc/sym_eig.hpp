// sym_eig.hpp -- interface of the host symmetric eigensolver (sym_eig.hip): plain C++, no HIP.
#pragma once
#include <cstdint>
#include <vector>

namespace gemhip {

// V (n x n, row-major, symmetric) is overwritten by the eigenvectors (columns); d gets the eigenvalues ASCENDING.  Timed and counted; a
// host-supplied solver, if one is set, is tried first from n = 64.  sym_eig_impl: the built-in solver itself.
void sym_eig(int n, std::vector<double> &V, std::vector<double> &d);
void sym_eig_impl(int n, std::vector<double> &V, std::vector<double> &d);
// Top-m eigenpairs: w DESCENDING, Z column-major n x m; G is overwritten.  Timed and counted.  sym_eig_top_impl: the partial solver itself.
void sym_eig_top(int n, std::vector<double> &G, int m, std::vector<double> &w, std::vector<double> &Z);
void sym_eig_top_impl(int n, std::vector<double> &V, int m, std::vector<double> &w, std::vector<double> &Z);
// Optional host-supplied eigensolver (e.g. LAPACK dsyevd through numpy): same contract as gemhip_sym_eig.  nullptr: none.
typedef int (*sym_eig_cb_t)(int32_t n, double *A_inout, double *w_out);
void set_sym_eig_callback(sym_eig_cb_t fn);
// Host threads of the O(n^3) phases: >= 1 sets them, <= 0 goes back to the default (GEMHIP_EIG_THREADS, else 1).  In effect: after the caps
// (16, half the cores this process may run on).
void set_eig_threads(int threads);
int eig_threads_in_effect();
// Wall time and number of the sym_eig / sym_eig_top calls since the last reset (a solve's statistics)
void reset_eig_stats();
double eig_seconds();
double eig_calls();

}  // namespace gemhip
