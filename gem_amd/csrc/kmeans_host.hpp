// kmeans_host.hpp -- the host arithmetic of the k-means handle (kmeans_host.hip): the check of the seeding's uniforms, the variance sklearn's
// tol is relative to, the padded centre block the assign kernel reads, the centres of an update from its fp64 sums, sklearn's relocation of empty clusters with its order fixed, the bookkeeping of the
// k-means++ draws, and the clustering scores (NMI, ARI, purity, homogeneity) of an integer contingency table.  The scans of the matrix and
// of label lists, and the zero-padded copy of the matrix, are the ones every evaluation unit shares: matrix_host.hpp.
// Plain C++, no HIP: everything here runs on a CPU (scripts/build_asan_kmeans.sh, tests/test_clustering.py); kmeans.hip words the refusals,
// uploads and launches.
#pragma once
#include <cstdint>
#include <vector>

namespace gemhip {

// The first t with u[t] outside [0, 1) (NaN included), or -1.
int64_t km_first_bad_uniform(const double *u, int64_t count);
// mean(var(X, axis=0)), fp64, two passes: what sklearn's tol is relative to.
double km_mean_variance(const float *X, int64_t n, int32_t d, int64_t ld);

// The centre block the assign kernel reads: Cp [Kp][dpad] = C [K][d] padded with zero columns and zero rows, cn [Kp] = |c_k|^2 summed in
// fp64 and rounded to fp32 once, +inf for the padding rows -- a padding centre never wins a comparison.
void km_pad_centres(int32_t K, int32_t d, int32_t dpad, int32_t Kp, const float *C, float *Cp, float *cn);

// C [K][d] = float32(sums[k][c] / counts[k]) from the update's sums [K][dpad]; a cluster of count 0 gets zeros.
void km_centres_from_sums(int32_t K, int32_t d, int32_t dpad, const double *sums, const int64_t *counts, float *C);
// sum_k |a_k - b_k|^2 in fp64, in index order.
double km_centre_shift(int32_t K, int32_t d, const float *a, const float *b);

// The rows sklearn's _relocate_empty_clusters_dense moves, its order fixed: the n_take rows of largest dist, descending, ties to the lower
// row id.  out [n_take].
void km_relocation_order(int64_t n, const double *dist, int64_t n_take, int64_t *out);
// Applies the relocation to an update's sums [K][dpad] and counts [K]: the j-th empty cluster in ascending id takes row rows[j] (its values
// xrows [n_empty][dpad], its label donor[j]); the row leaves its donor's sum and count.  Returns -1, or the first j whose donor would be left
// without a row (nothing is divided by zero: the caller refuses).
int64_t km_relocate(int32_t K, int32_t dpad, const std::vector<int32_t> &empty, const int32_t *donor, const float *xrows, double *sums, int64_t *counts);

// k-means++ draws.  The first centre: row min(floor(u n), n - 1).
int64_t km_first_row(double u, int64_t n);
// searchsorted(cumsum(D2), v, side='right') by blocks: prefix [nb + 1] is the running fp64 sum of the block sums (prefix[0] = 0).  Returns the
// first block whose closing prefix exceeds v (nb if none does).
int64_t km_find_block(const double *prefix, int64_t nb, double v);
// Within a block: start is the prefix before it, vals its len D2 values in row order.  The first t with start + vals[0] + ... + vals[t] > v, or -1.
int64_t km_find_in_block(double start, const float *vals, int64_t len, double v);

// out[4] = {NMI (arithmetic mean of the entropies; 1 when both partitions are a single cluster), ARI (pair counts in 128-bit integers),
// purity, homogeneity} of table [Kp][Kt] (rows: predicted clusters, columns: true classes), all fp64 from the integers.  Empty rows and
// columns are legal.  Returns false for a negative entry or an empty table.
bool km_scores(const int64_t *table, int32_t Kp, int32_t Kt, double *out);

}  // namespace gemhip
