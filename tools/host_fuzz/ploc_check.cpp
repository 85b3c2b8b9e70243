// evplp_ploc_tree (csrc/host/ploc.cpp) over its edge cases and over seeded random triangle soups -- 0, 1, 2, 5 triangles, fewer triangles than
// the radius, 64 copies of one triangle (every key and every distance ties), triangles without area among valid ones, coordinates that are not
// finite, every radius 1 .. 32 and search-iteration counts 0 .. 128 -- for tests/test_ploc_host.py, which builds it with AddressSanitizer +
// UndefinedBehaviorSanitizer: a valid tree within the iteration bound, or a refusal; never a loop and never an access outside the arrays.
#include "evplp.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>
static long trees = 0, refused = 0;
// n valid of ntri: every inner node but 0 and every leaf is a child exactly once, children lie above their parents, order is a permutation of valid triangles
static void check(const std::vector<float> &v, int ntri, int radius, int search, int expect_n) {
    std::vector<int32_t> order((size_t)(ntri > 0 ? ntri : 1), -7), children((size_t)(ntri > 1 ? 2 * (ntri - 1) : 1), -7);
    int32_t it = -1;
    const int n = evplp_ploc_tree(ntri > 0 ? v.data() : nullptr, ntri, radius, search, order.data(), children.data(), &it);
    if (n < 0) { fprintf(stderr, "refused: ntri %d radius %d search %d\n", ntri, radius, search); exit(1); }
    if (expect_n >= 0 && n != expect_n) { fprintf(stderr, "n = %d, expected %d\n", n, expect_n); exit(1); }
    int lg = 0; while ((1 << lg) < n) lg++;
    if (it < 0 || it > search + lg || (n > 1 && it < 1)) { fprintf(stderr, "iterations %d for n %d search %d\n", it, n, search); exit(1); }
    std::vector<int> seen_tri((size_t)(ntri > 0 ? ntri : 1), 0), as_child((size_t)(n > 1 ? 2 * n - 1 : 1), 0);
    for (int p = 0; p < n; p++) { if (order[p] < 0 || order[p] >= ntri || seen_tri[order[p]]++) { fprintf(stderr, "order\n"); exit(1); } }
    for (int i = 0; i + 1 < n; i++) for (int s = 0; s < 2; s++) {
        const int32_t c = children[2 * i + s];
        if (c >= 0 ? (c <= i || c > n - 2) : (~c >= n)) { fprintf(stderr, "child %d of node %d (n %d)\n", c, i, n); exit(1); }
        if (as_child[c >= 0 ? c : n - 1 + ~c]++) { fprintf(stderr, "child %d twice\n", c); exit(1); }
    }
    for (int k = 1; k < 2 * n - 1 && n > 1; k++) if (!as_child[k]) { fprintf(stderr, "node / leaf %d has no parent\n", k); exit(1); }
    trees++;
}
int main() {
    std::mt19937 rng(4);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    auto tri = [&](std::vector<float> &v, float x, float y, float z, float s) { const float t[9] = { x, y, z, x + s, y, z + 0.1f * s, x, y + s, z }; v.insert(v.end(), t, t + 9); };
    const int radii[] = { 1, 2, 5, 16, 32 }, searches[] = { 0, 1, 3, 128 };
    for (int r : radii) for (int s : searches) {
        for (int n : { 0, 1, 2, 5, 17, 33 }) {                                  // (n <= r: the window covers everything)
            std::vector<float> v; for (int k = 0; k < n; k++) tri(v, (float)k + 0.5f * u(rng), u(rng), u(rng), 0.3f);
            check(v, n, r, s, n);
        }
        { std::vector<float> v; for (int k = 0; k < 64; k++) tri(v, 0.1f, 0.2f, 0.3f, 1.0f); check(v, 64, r, s, 64); }
        {   // without area, not finite, and valid ones between them
            std::vector<float> v; const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
            tri(v, 0, 0, 0, 1); tri(v, 1, 1, 1, 0); tri(v, 2, 0, 0, 1); tri(v, inf, 0, 0, 1); tri(v, 0, nan, 0, 1); tri(v, 3, 1, 0, 1); tri(v, 3.0e38f, 0, 0, 3.0e38f); tri(v, 1, 2, 3, 1e-30f);
            check(v, 8, r, s, -1);
        }
    }
    for (int it = 0; it < 300; it++) {                                         // random soups: clusters, duplicates, a few thousand triangles at most
        const int n = 1 + (int)(rng() % (it < 280 ? 300 : 3000)), r = 1 + (int)(rng() % 32), s = (int)(rng() % 129);
        std::vector<float> v;
        for (int k = 0; k < n; k++) {
            if (k > 0 && rng() % 5 == 0) { v.insert(v.end(), v.end() - 9, v.end()); continue; }      // (a copy of the one before)
            tri(v, 10.f * u(rng), rng() % 3 ? u(rng) : 0.5f, u(rng), rng() % 11 ? 0.05f + u(rng) : 0.f);
        }
        check(v, n, r, s, -1);
    }
    {   // refusals
        std::vector<float> v; tri(v, 0, 0, 0, 1); tri(v, 1, 0, 0, 1);
        int32_t o[2], c[2], it;
        const int rc[] = { evplp_ploc_tree(nullptr, 2, 16, 128, o, c, &it), evplp_ploc_tree(v.data(), 2, 0, 128, o, c, &it), evplp_ploc_tree(v.data(), 2, 33, 128, o, c, &it),
                           evplp_ploc_tree(v.data(), 2, 16, 129, o, c, &it), evplp_ploc_tree(v.data(), 2, 16, -1, o, c, &it), evplp_ploc_tree(v.data(), -1, 16, 128, o, c, &it),
                           evplp_ploc_tree(v.data(), 2, 16, 128, nullptr, c, &it), evplp_ploc_tree(v.data(), 2, 16, 128, o, nullptr, &it), evplp_ploc_tree(v.data(), 2, 16, 128, o, c, nullptr) };
        for (int x : rc) { if (x != EVPLP_ERR_INVALID) { fprintf(stderr, "not refused\n"); return 1; } refused++; }
    }
    printf("trees %ld refused %ld\n", trees, refused);
    return 0;
}
