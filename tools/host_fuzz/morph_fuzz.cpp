// evplp_morph_points and the loops behind evplp_morph_mesh (csrc/host/morph.cpp) over seeded random argument sets -- valid targets of 1 .. 64
// planes with weights of any finite value, and every way the call refuses: null pointers, target counts outside 1 .. 64, a negative point
// count, deltas, weights and points that are not finite, products that overflow -- for tests/test_morph_host.py, which builds it with
// AddressSanitizer + UndefinedBehaviorSanitizer.  The arrays are exactly as long as the call may read: a stride or a count that is off
// reads outside them and the sanitizer sees it.  A refused call leaves out untouched; an accepted one gives finite points, the input value
// for value under all-zero weights, and p + d_k exactly under one weight of 1 over quarters.  morph_deform is then run on the result under
// nothing, a translation and a palette of two translations, as evplp_morph_mesh composes them for the host copy of a mesh.
#include "evplp.h"
#include "morph.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
int main() {
    std::mt19937 rng(23);
    std::uniform_real_distribution<float> coord(-10.0f, 10.0f), weight(-2.0f, 3.0f);
    long ok = 0, bad = 0, composed = 0;
    for (int it = 0; it < 6000; it++) {
        const int T = (it % 40 == 0) ? 64 : 1 + (int)(rng() % 9);
        const int n = (int)(rng() % 40);
        const int mode = (int)(rng() % 3);          // 0: anything, 1: all-zero weights, 2: quarters and one weight of 1
        const int one = (int)(rng() % (unsigned)T);
        std::vector<float> d(3 * (size_t)n * (size_t)T), w((size_t)T), in(3 * (size_t)n), out(3 * (size_t)n, -77.0f);
        for (auto &v : in) v = mode == 2 ? (float)((int)(rng() % 129) - 64) * 0.25f : coord(rng);
        for (auto &v : d) v = mode == 2 ? (float)((int)(rng() % 129) - 64) * 0.25f : coord(rng) * 0.1f;
        for (int k = 0; k < T; k++) w[(size_t)k] = mode == 0 ? weight(rng) : (mode == 2 && k == one) ? 1.0f : 0.0f;
        // one in two argument sets is spoilt in one way
        const unsigned spoil = rng() % 2 ? 1 + rng() % 9 : 0;
        int tt = T, nn = n;
        const float *pd = d.data(), *pw = w.data(), *pin = in.data(); float *pout = out.data();
        bool expect_bad = false;
        switch (spoil) {
        case 1: pw = nullptr; expect_bad = true; break;
        case 2: if (n > 0) { pd = nullptr; expect_bad = true; } break;
        case 3: if (n > 0) { if (rng() % 2) pin = nullptr; else pout = nullptr; expect_bad = true; } break;
        case 4: tt = rng() % 2 ? 0 - (int)(rng() % 3) : 65 + (int)(rng() % 5); expect_bad = true; break;     // (refused before any array is read)
        case 5: nn = -1 - (int)(rng() % 5); expect_bad = true; break;
        case 6: if (n > 0) { d[rng() % d.size()] = rng() % 2 ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity(); expect_bad = true; } break;
        case 7: w[rng() % w.size()] = rng() % 2 ? std::numeric_limits<float>::quiet_NaN() : -std::numeric_limits<float>::infinity(); expect_bad = true; break;
        case 8: if (n > 0) { in[rng() % in.size()] = std::numeric_limits<float>::quiet_NaN(); expect_bad = true; } break;
        case 9: if (n > 0) { const size_t v = rng() % (size_t)n; d[3 * ((size_t)(T - 1) * (size_t)n + v)] = 3.0e38f; w[(size_t)T - 1] = 3.0e38f; expect_bad = true; } break;
        default: break;
        }
        const int rc = evplp_morph_points(pin, pd, pw, tt, nn, pout);
        if ((rc < 0) != expect_bad) { std::printf("BAD VERDICT it %d spoil %u rc %d\n", it, spoil, rc); return 1; }
        if (rc < 0) {
            if (rc != EVPLP_ERR_INVALID) { std::puts("BAD CODE"); return 1; }
            for (float v : out) if (v != -77.0f) { std::puts("A REFUSAL WROTE"); return 1; }
            bad++; continue;
        }
        ok++;
        for (int v = 0; v < n; v++) for (int r = 0; r < 3; r++) {
            const size_t at = 3 * (size_t)v + r;
            const float got = out[at];
            if (!std::isfinite(got)) { std::puts("BAD POINT"); return 1; }
            if (mode == 1 && got != in[at]) { std::puts("BAD ZERO WEIGHTS"); return 1; }
            if (mode == 2 && got != in[at] + d[3 * ((size_t)one * (size_t)n) + at]) { std::puts("BAD UNIT WEIGHT"); return 1; }
        }
        // in place: the same points
        std::vector<float> again(in);
        if (evplp_morph_points(again.data(), pd, pw, tt, nn, again.data()) != EVPLP_OK || (n > 0 && std::memcmp(again.data(), out.data(), sizeof(float) * out.size()) != 0)) { std::puts("BAD IN PLACE"); return 1; }
        // the composition for the host copy: the base under nothing, under a matrix, under a palette over a skin
        if (n > 0 && it % 4 == 0) {
            const float shift[12] = { 1, 0, 0, 0.5f, 0, 1, 0, -2.0f, 0, 0, 1, 4.0f };
            float pal[24]; std::memcpy(pal, shift, sizeof(shift)); std::memcpy(pal + 12, shift, sizeof(shift)); pal[12 + 3] = 1.5f;
            std::vector<int32_t> bi(4 * (size_t)n, 0); std::vector<float> bw(4 * (size_t)n, 0.0f);
            for (int v = 0; v < n; v++) { bi[4 * (size_t)v] = (int32_t)(rng() % 2); bw[4 * (size_t)v] = 1.0f; }
            std::vector<float> a(out.size()), b(out.size()), c(out.size());
            if (evplp::morph_deform(out.data(), nullptr, nullptr, nullptr, nullptr, a.data(), (size_t)n) >= 0 || std::memcmp(a.data(), out.data(), sizeof(float) * a.size()) != 0) { std::puts("BAD COPY"); return 1; }
            if (evplp::morph_deform(out.data(), shift, nullptr, nullptr, nullptr, b.data(), (size_t)n) >= 0) { std::puts("BAD MATRIX"); return 1; }
            if (evplp::morph_deform(out.data(), nullptr, pal, bi.data(), bw.data(), c.data(), (size_t)n) >= 0) { std::puts("BAD POSE"); return 1; }
            for (int v = 0; v < n; v++) {
                if (b[3 * (size_t)v + 1] != out[3 * (size_t)v + 1] + -2.0f) { std::puts("BAD SHIFT"); return 1; }
                if (c[3 * (size_t)v] != out[3 * (size_t)v] + (bi[4 * (size_t)v] ? 1.5f : 0.5f)) { std::puts("BAD PALETTE"); return 1; }
            }
            float huge[12] = { 3.0e38f, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
            out[0] = 8.0f;
            if (evplp::morph_deform(out.data(), huge, nullptr, nullptr, nullptr, b.data(), (size_t)n) != 0) { std::puts("BAD OVERFLOW"); return 1; }
            composed++;
        }
    }
    std::printf("morphed %ld refused %ld composed %ld\n", ok, bad, composed);
    return 0;
}
