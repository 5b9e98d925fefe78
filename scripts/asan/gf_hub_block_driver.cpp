// Stand-alone driver of the blocked hub-row arithmetic in gem_amd/csrc/gf_plan.hip: plain C++, no HIP, no device.
//
//   gf_hub_block_driver block <d>...
//       stdout: one line "<d> <row floats> <B>" per width (0 0 for a width the GF dispatch does not support)
//   gf_hub_block_driver decay <eta> <regu> <B>
//       eta, regu: decimal floats (9 significant digits name an fp32 value exactly).  stdout: B + 1 lines "<k> <bits of hi[k]> <bits of lo[k]>",
//       the fp32 bit patterns as unsigned decimals (tests/test_gf_hub_block.py compares hi + lo with numpy's fp64 powers)
#include "../../gem_amd/csrc/gf_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace gemhip;

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "block")) {
        for (int k = 2; k < argc; ++k) {
            const int d = atoi(argv[k]);
            printf("%d %d %d\n", d, gf_row_floats(d), gf_hub_block(d));
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "decay")) {
        const float eta = strtof(argv[2], nullptr), regu = strtof(argv[3], nullptr);
        const int B = atoi(argv[4]);
        if (B < 1 || B > GF_HUB_BLOCK_MAX) { fprintf(stderr, "gf_hub_block_driver: B=%d outside 1..%d\n", B, GF_HUB_BLOCK_MAX); return 2; }
        std::vector<float> hi(B + 1), lo(B + 1);
        gf_hub_decay(eta, regu, B, hi.data(), lo.data());
        for (int k = 0; k <= B; ++k) {
            uint32_t h, l;
            memcpy(&h, &hi[k], 4); memcpy(&l, &lo[k], 4);
            printf("%d %u %u\n", k, h, l);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s block <d>... | decay <eta> <regu> <B>\n", argv[0]);
    return 2;
}
