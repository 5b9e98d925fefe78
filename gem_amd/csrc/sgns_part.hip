// sgns_part.hip -- the partitioned-table instantiations of sgns_win_kernel (sgns.hpp, PART): TrainModel in walk order restricted to ONE bucket
// (contexts of SynPos partition g, centre words and negatives of SynNeg partition h) of the N-GPU episode schedule (DESIGN.md section 6,
// gemhip_sgns_train_part).  Hogwild (delta write-back + reload-on-update) for the product path, overwrite-on-leave on one wavefront for the parity tests.
#include "sgns.hpp"

namespace gemhip {
sgns_fn pick_sgns_win_part(int d, bool hogwild)
{
    if (hogwild) return sgns_pick_width(d, [](auto vec, auto nv) -> sgns_fn { return launch_sgns_win_part<vec(), nv(), true>; });
    return sgns_pick_width(d, [](auto vec, auto nv) -> sgns_fn { return launch_sgns_win_part<vec(), nv(), false>; });
}
}  // namespace gemhip
