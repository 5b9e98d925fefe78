// sgns_hogwild.hip -- the Hogwild instantiations of sgns_win_kernel (sgns.hpp): one wavefront per walk, LDS window with delta write-back,
// reload-on-update of the negative rows, hot rows kept out of the window.  What gemhip_sgns_train launches unless flags|4 (deterministic).
#include "sgns.hpp"

namespace gemhip {
sgns_fn pick_sgns_win_hogwild(int d)
{
    return sgns_pick_width(d, [](auto vec, auto nv) -> sgns_fn { return launch_sgns_win<vec(), nv(), true>; });
}
}  // namespace gemhip
