// Driver of scripts/build_tsan_eig.sh: the partial and the full built-in solver of gem_amd/csrc/sym_eig.hip at 2, 3 and 4 host threads.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include <cmath>
#include "../../gem_amd/csrc/sym_eig.hpp"
using namespace gemhip;
int main()
{
    uint64_t s = 12345;
    auto rnd = [&]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)((s >> 11) & 0xFFFFFFFFFFFFFull) / 4503599627370496.0 - 0.5; };
    for (int kind = 0; kind < 3; ++kind)
        for (int n : {192, 257, 320}) {
            std::vector<double> A((size_t)n * n, 0.0);
            if (kind == 0) { for (int i = 0; i < n; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = rnd(); }
            else if (kind == 1) { for (int i = 0; i < n; ++i) A[(size_t)i * n + i] = 1.0 + i; }
            else { int k = n / 2; for (int i = 0; i < k; ++i) for (int j = 0; j <= i; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = rnd(); }
            for (int T : {2, 3, 4}) {
                set_eig_threads(T);
                std::vector<double> B(A), w, Z;
                sym_eig_top_impl(n, B, 40, w, Z);
                std::vector<double> C(A), wf;
                sym_eig_impl(n, C, wf);
                printf("kind %d n %d T %d  top %.6f  full-top %.6f\n", kind, n, eig_threads_in_effect(), w[0], wf[n - 1]);
                if (std::fabs(w[0] - wf[n - 1]) > 1e-9 * (1 + std::fabs(w[0]))) return 1;
            }
        }
    return 0;
}
