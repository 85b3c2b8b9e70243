// evplp_refit_levels (csrc/host/refit_levels.cpp) over seeded random node arrays -- trees, forests, cycles, shared children, child indices
// past the end, capacities too small -- for tests/test_refit_host.py, which builds it with AddressSanitizer + UndefinedBehaviorSanitizer: a plan
// or a refusal, never a loop and never an access outside the arrays.
#include "evplp.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
int main() {
    std::mt19937 rng(1);
    long ok = 0, bad = 0;
    for (int it = 0; it < 200000; it++) {
        int n = 1 + rng() % 12;
        std::vector<unsigned char> nodes(64 * n, 0);
        for (int i = 0; i < n; i++) for (int s = 0; s < 2; s++) {
            int32_t c; unsigned r = rng() % 10;
            if (r < 4) c = -1 - (int32_t)(rng() % 100); else if (r == 4) c = INT32_MIN; else if (r == 5) c = n + (int32_t)(rng() % 3); else c = (int32_t)(rng() % n);
            std::memcpy(&nodes[64 * i + 48 + 4 * s], &c, 4);
        }
        int cap = 1 + rng() % 8;
        std::vector<int32_t> h(n), o(n), b(cap + 1);
        int rc = evplp_refit_levels(nodes.data(), n, h.data(), o.data(), b.data(), cap);
        if (rc > 0) { ok++; if (b[rc] > n || rc > cap) { std::puts("BAD PLAN"); return 1; } } else bad++;
    }
    std::printf("plans %ld refused %ld\n", ok, bad);
    return 0;
}
