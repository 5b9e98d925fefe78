// rank_host.hpp -- the device-free half of the binary ranking metrics (rank_host.hip): the order-preserving key of an fp64 score, the input
// checks, which radix passes a digit histogram lets the sort skip, and ROC-AUC / average precision from the table of tie groups.
// Plain C++, no HIP: everything here runs on a CPU (scripts/build_asan_rank.sh, tests/test_link_auc.py); rank.hip words the refusals,
// uploads and launches.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RANK_HD __host__ __device__ inline
#else
#define RANK_HD inline
#endif

namespace gemhip {

constexpr int RANK_RADIX_BITS = 8;
constexpr int RANK_PASSES = 64 / RANK_RADIX_BITS;
constexpr int RANK_BUCKETS = 1 << RANK_RADIX_BITS;

// Ascending order of the key = descending order of the score: the usual sign-flip transform, inverted, -0.0 first made +0.0 (the two zeros
// are one tie group, as in sklearn).  +inf gets the smallest key, -inf the largest; NaN never gets here.
RANK_HD uint64_t rank_key_of_bits(uint64_t b)
{
    if (b == 0x8000000000000000ull) b = 0;
    const uint64_t asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return ~asc;
}
RANK_HD uint64_t rank_bits_of_key(uint64_t key)
{
    const uint64_t asc = ~key;
    return (asc >> 63) ? (asc & 0x7fffffffffffffffull) : ~asc;
}
inline uint64_t rank_key(double s)
{
    uint64_t b;
    std::memcpy(&b, &s, 8);
    return rank_key_of_bits(b);
}
inline double rank_score_of_key(uint64_t key)
{
    const uint64_t b = rank_bits_of_key(key);
    double s;
    std::memcpy(&s, &b, 8);
    return s;
}

// The first t with score[t] NaN, or -1.
int64_t rank_first_nan(const double *score, int64_t m);
// The first t with label[t] neither 0 nor 1, or -1.
int64_t rank_first_bad_label(const uint8_t *label, int64_t m);
// hist [RANK_PASSES][RANK_BUCKETS]: how many of the m keys have each digit, per pass (pass 0 = the lowest byte).  active[p] = the pass moves
// something, i.e. more than one bucket of it is non-empty.  Returns the number of active passes.
int rank_active_passes(const uint32_t *hist, int64_t m, bool *active);

enum RankGroupError { RANK_OK = 0, RANK_EMPTY, RANK_NOT_CUMULATIVE, RANK_NO_POSITIVE, RANK_NO_NEGATIVE };
// tp [T], fp [T]: the cumulative positives / negatives at the end of each tie group, descending score.  out [4] = {auc, ap, prevalence, 0},
// counts [4] = {P, N, T, U2}:  U2 = sum_g pos_g (2 (N - fp_g) + neg_g), an exact integer, twice the Mann-Whitney U; auc = U2 / (2 P N), one
// fp64 division; ap = (1 / P) sum_g pos_g tp_g / (tp_g + fp_g) with fp64 terms summed in group order.  *bad_group: the offender of
// RANK_NOT_CUMULATIVE (tp or fp decreases, a group is empty, or the totals reach 2^31).
RankGroupError rank_from_groups(int64_t T, const int64_t *tp, const int64_t *fp, double *out, int64_t *counts, int64_t *bad_group);

// One term of the sums above, shared with the device (rank.hip): the same expression, so the same bits per term.
RANK_HD int64_t rank_u2_term(int64_t pos, int64_t neg, int64_t fp_end, int64_t N) { return pos * (2 * (N - fp_end) + neg); }
RANK_HD double rank_ap_term(int64_t pos, int64_t tp_end, int64_t fp_end) { return (double)pos * ((double)tp_end / (double)(tp_end + fp_end)); }

}  // namespace gemhip
