// evplp_rotate_tree (csrc/host/rotate.cpp) over seeded random node arrays -- trees of 1 .. 300 nodes with leaf references into (and past) a
// small triangle array, absent children, triangles without area, and arrays that are no trees at all -- for tests/test_rotate_host.py,
// which builds it with AddressSanitizer + UndefinedBehaviorSanitizer: a rotated tree over the same nodes and leaf references whose every
// inner child lies on a lower plan level than its parent, or a refusal; never a loop and never an access outside the arrays.
#include "evplp.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
int main() {
    std::mt19937 rng(4);
    long ok = 0, bad = 0, taken = 0;
    for (int it = 0; it < 20000; it++) {
        const int n = (it % 40 == 0) ? 1 + (int)(rng() % 300) : 1 + (int)(rng() % 14);
        const bool tree = rng() % 4 != 0;                 // three quarters are trees by construction (node i's inner children lie behind i)
        const int nblocks = 1 + (int)(rng() % 40), ntri = (int)(rng() % 120);
        std::vector<unsigned char> nodes(64 * (size_t)n, 0);
        std::vector<int32_t> tri_index(4 * (size_t)nblocks);
        for (auto &t : tri_index) t = rng() % 8 == 0 ? -1 : (int32_t)(rng() % (ntri + 3)) - 1;      // (some past the end, some -1)
        std::vector<float> verts(9 * (size_t)std::max(ntri, 1));
        for (int t = 0; t < ntri; t++) {
            const bool flat = rng() % 10 == 0;
            for (int k = 0; k < 9; k++) verts[9 * (size_t)t + k] = flat ? 1.0f : (float)(rng() % 2001) * 0.01f - 10.0f;
        }
        int next = 1;
        for (int i = 0; i < n; i++) for (int s = 0; s < 2; s++) {
            int32_t c; const unsigned r = rng() % 10;
            if (tree) c = (r < 6 && next < n) ? next++ : r == 9 ? INT32_MIN : ~(int32_t)(rng() % (4 * (unsigned)nblocks + 8));
            else if (r < 4) c = -1 - (int32_t)(rng() % 100); else if (r == 4) c = INT32_MIN; else if (r == 5) c = n + (int32_t)(rng() % 3); else c = (int32_t)(rng() % n);
            std::memcpy(&nodes[64 * (size_t)i + 48 + 4 * s], &c, 4);
        }
        const int passes = 1 + (int)(rng() % 8);
        std::vector<int32_t> kids(2 * (size_t)n, 0), rot(8, -1), height((size_t)n), order((size_t)n), begin((size_t)n + 1);
        std::vector<float> boxes(6 * (size_t)n);
        int32_t need0 = -1;
        const int levels0 = evplp_refit_levels(nodes.data(), n, height.data(), order.data(), begin.data(), n);
        const int rc = evplp_rotate_tree(nodes.data(), n, tri_index.data(), 4 * nblocks, verts.data(), ntri, nullptr, passes, kids.data(), boxes.data(), rot.data(), &need0);
        if ((rc < 0) != (levels0 < 0)) { std::puts("BAD REFUSAL"); return 1; }
        if (rc < 0) { bad++; continue; }
        ok++;
        if (rc != levels0 || need0 < 0) { std::puts("BAD LEVELS"); return 1; }
        // the plan is still a schedule, and the leaf references are a permutation of what they were
        std::vector<int32_t> before, after;
        for (int e = 0; e < begin[(size_t)levels0]; e++) {
            const int32_t i = order[(size_t)e];
            for (int s = 0; s < 2; s++) {
                int32_t c0; std::memcpy(&c0, &nodes[64 * (size_t)i + 48 + 4 * s], 4);
                const int32_t c1 = kids[2 * (size_t)i + s];
                if (c0 < 0) before.push_back(c0);
                if (c1 < 0) after.push_back(c1);
                else if (c1 >= n || height[(size_t)c1] < 0 || !(height[(size_t)c1] < height[(size_t)i])) { std::puts("BAD LEVEL ORDER"); return 1; }
            }
        }
        std::sort(before.begin(), before.end()); std::sort(after.begin(), after.end());
        if (before != after) { std::puts("BAD LEAVES"); return 1; }
        std::vector<unsigned char> again(nodes);
        for (int i = 0; i < n; i++) std::memcpy(&again[64 * (size_t)i + 48], &kids[2 * (size_t)i], 8);
        if (evplp_refit_levels(again.data(), n, height.data(), order.data(), begin.data(), n) < 1 || begin[1] < 1) { std::puts("BAD TREE"); return 1; }
        for (int p = 0; p < passes; p++) { if (rot[(size_t)p] < 0 || rot[(size_t)p] > n) { std::puts("BAD COUNT"); return 1; } taken += rot[(size_t)p]; }
    }
    std::printf("rotated %ld refused %ld rotations %ld\n", ok, bad, taken);
    return 0;
}
