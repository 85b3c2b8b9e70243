// evplp_accel_cost (csrc/host/accel_cost.cpp) over seeded random node arrays -- trees of 1 .. 700 nodes (so up to three chunks of 256, most
// with a ragged last one), forests, cycles, shared children, child indices past the end, absent children, empty boxes -- for
// tests/test_accel_quality_host.py, which builds it with AddressSanitizer + UndefinedBehaviorSanitizer: five finite figures that agree with
// a plain running sum of the same terms, or a refusal; never a loop and never an access outside the arrays.
#include "evplp.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
int main() {
    std::mt19937 rng(2);
    long ok = 0, bad = 0;
    for (int it = 0; it < 20000; it++) {
        const int n = (it % 50 == 0) ? 1 + (int)(rng() % 700) : 1 + (int)(rng() % 12);
        const bool tree = rng() % 2 == 0;                 // half of the arrays are trees by construction (node i's inner children lie behind i)
        std::vector<unsigned char> nodes(64 * (size_t)n, 0);
        int next = 1;
        for (int i = 0; i < n; i++) for (int s = 0; s < 2; s++) {
            int32_t c; const unsigned r = rng() % 10;
            if (tree) c = (r < 6 && next < n) ? next++ : r == 9 ? INT32_MIN : ~(int32_t)(rng() % 4096);
            else if (r < 4) c = -1 - (int32_t)(rng() % 100); else if (r == 4) c = INT32_MIN; else if (r == 5) c = n + (int32_t)(rng() % 3); else c = (int32_t)(rng() % n);
            std::memcpy(&nodes[64 * (size_t)i + 48 + 4 * s], &c, 4);
            for (int k = 0; k < 3; k++) {
                const float ctr = (float)(rng() % 2001) * 0.01f - 10.0f, hal = (c == INT32_MIN || rng() % 40 == 0) ? -3.0e38f : (float)(rng() % 1000) * 0.003f;
                std::memcpy(&nodes[64 * (size_t)i + 8 * k + 4 * s], &ctr, 4);
                std::memcpy(&nodes[64 * (size_t)i + 24 + 8 * k + 4 * s], &hal, 4);
            }
        }
        double out[5] = { -1, -1, -1, -1, -1 };
        const int rc = evplp_accel_cost(nodes.data(), n, out);
        if (rc < 0) { bad++; continue; }
        ok++;
        if (rc > n) { std::puts("BAD COUNT"); return 1; }
        // the same terms in a running sum over the reached nodes, in whatever order a walk from the root finds them
        double want[3] = { 0, 0, 0 };
        std::vector<int32_t> stack(1, 0);
        int reached = 0;
        while (!stack.empty()) {
            const int32_t i = stack.back(); stack.pop_back(); reached++;
            for (int s = 0; s < 2; s++) {
                int32_t c; std::memcpy(&c, &nodes[64 * (size_t)i + 48 + 4 * s], 4);
                float h[3]; for (int k = 0; k < 3; k++) std::memcpy(&h[k], &nodes[64 * (size_t)i + 24 + 8 * k + 4 * s], 4);
                if (c >= 0) stack.push_back(c);
                if (c == INT32_MIN || h[0] < 0 || h[1] < 0 || h[2] < 0) continue;
                const double a = 8.0 * ((double)h[0] * h[1] + (double)h[1] * h[2] + (double)h[2] * h[0]);
                if (c >= 0) want[0] += a; else { const int cnt = (~c & 3) + 1; want[1] += a * ((cnt + 1) >> 1); want[2] += a * cnt; }
            }
        }
        if (reached != rc) { std::puts("BAD REACH"); return 1; }
        for (int j = 0; j < 3; j++)
            if (!(std::fabs(out[2 + j] - want[j]) <= 1e-12 * want[j])) { std::printf("BAD SUM %d: %.17g vs %.17g (n %d)\n", j, out[2 + j], want[j], n); return 1; }
        const double cost = out[1] > 0 ? (15.0 * (out[1] + out[2]) + 40.0 * out[3]) / out[1] : 0.0;
        if (!(out[1] >= 0) || !std::isfinite(out[0]) || out[0] != cost) { std::printf("BAD COST %.17g vs %.17g\n", out[0], cost); return 1; }
    }
    std::printf("costs %ld refused %ld\n", ok, bad);
    return 0;
}
