// matrix_host.hpp -- the device-free checks every evaluation unit makes of what it ingests (matrix_host.hip): the scan of an embedding
// matrix for an entry it must refuse, the zero-padded copy of its live columns, and the scans of index and pair lists.
// Plain C++, no HIP: everything here runs on a CPU (scripts/asan/matrix_host_driver.cpp, tests/test_matrix_host.py).  The functions return
// positions; the .hip unit that calls them words the refusal (eval_common.hpp words the ones all units share).
#pragma once
#include <cstdint>

namespace gemhip {

// The flat position i * d + c of the first X[i][c < d] that is not finite or whose magnitude exceeds max_abs, or -1.  X [n][ld]; the
// columns d <= c < ld are never read.  max_abs = INFINITY checks finiteness only; a magnitude equal to max_abs passes.
int64_t first_bad_entry(const float *X, int64_t n, int32_t d, int64_t ld, float max_abs);
// out [n][dpad] = the columns c < d of X [n][ld], zeros in d <= c < dpad.  dpad >= d.
void pad_rows(const float *X, int64_t n, int32_t d, int64_t ld, int32_t dpad, float *out);
// The first t with idx[t] outside [0, n), or -1.
int64_t first_bad_index(const int32_t *idx, int64_t m, int64_t n);
// The first p with st[p] or ed[p] outside [0, n), or -1.
int64_t first_bad_pair(const int32_t *st, const int32_t *ed, int64_t m, int64_t n);

}  // namespace gemhip
