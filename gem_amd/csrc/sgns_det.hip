// sgns_det.hip -- the deterministic instantiations (sgns.hpp): sgns_win_kernel with overwrite on leave and sgns_kernel (no LDS window).
// One wavefront of either reproduces oracle/n2v_oracle.c to 2e-4; sgns_kernel is also the Hogwild fallback for d >= 384 (window does not fit).
#include "sgns.hpp"

namespace gemhip {
sgns_fn pick_sgns_win_det(int d)
{
    return sgns_pick_width(d, [](auto vec, auto nv) -> sgns_fn { return launch_sgns_win<vec(), nv(), false>; });
}

sgns_fn pick_sgns(int d)
{
    return sgns_pick_width(d, [](auto vec, auto nv) -> sgns_fn { return launch_sgns<vec(), nv()>; });
}
}  // namespace gemhip
