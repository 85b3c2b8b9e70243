// evplp_skin_points (csrc/host/skin.cpp) over seeded random argument sets -- valid skins over palettes of 1 .. 1024 bones, and every way
// the call refuses: null pointers, bone counts outside 1 .. 1024, indices outside the palette (also under a zero weight), weights that are
// negative, not finite or do not add up to 1, matrix entries that are not finite, products that overflow -- for tests/test_skin_host.py,
// which builds it with AddressSanitizer + UndefinedBehaviorSanitizer.  The arrays are exactly as long as the call may read: an index that
// slipped past the validation reads outside the palette and the sanitizer sees it.  A refused call leaves out untouched; an accepted one
// gives finite points, and under weights (1, 0, 0, 0) and a palette of translations the points moved by bone b[0]'s translation.
#include "evplp.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> coord(-10.0f, 10.0f), unit(0.0f, 1.0f);
    long ok = 0, bad = 0;
    for (int it = 0; it < 6000; it++) {
        const int nbones = (it % 50 == 0) ? 1024 : 1 + (int)(rng() % 12);
        const int n = (int)(rng() % 40);
        const bool translations = rng() % 3 == 0;
        std::vector<float> bones(12 * (size_t)nbones), w(4 * (size_t)n), in(3 * (size_t)n), out(3 * (size_t)n, -77.0f);
        std::vector<int32_t> idx(4 * (size_t)n);
        for (int b = 0; b < nbones; b++)
            for (int k = 0; k < 12; k++) bones[12 * (size_t)b + k] = translations ? (k % 4 == 3 ? (float)(b + k) : (k % 5 == 0 ? 1.0f : 0.0f)) : coord(rng) * 0.2f;
        for (auto &v : in) v = coord(rng);
        for (int v = 0; v < n; v++) {
            float sum = 0.0f;
            for (int k = 0; k < 4; k++) { idx[4 * (size_t)v + k] = (int32_t)(rng() % (unsigned)nbones); w[4 * (size_t)v + k] = (translations || rng() % 4 == 0) ? 0.0f : unit(rng); sum += w[4 * (size_t)v + k]; }
            if (translations || !(sum > 0.0f)) { for (int k = 0; k < 4; k++) w[4 * (size_t)v + k] = k == 0 ? 1.0f : 0.0f; }
            else for (int k = 0; k < 4; k++) w[4 * (size_t)v + k] /= sum;
        }
        // one in two argument sets is spoilt in one way
        const unsigned spoil = rng() % 2 ? 1 + rng() % 12 : 0;
        int nb = nbones, nn = n;
        const float *pb = bones.data(), *pw = w.data(), *pin = in.data(); const int32_t *pi = idx.data(); float *pout = out.data();
        bool expect_bad = false;
        const size_t slot = n > 0 ? rng() % (4 * (size_t)n) : 0;
        switch (spoil) {
        case 1: pb = nullptr; expect_bad = true; break;
        case 2: if (n > 0) { pi = nullptr; expect_bad = true; } break;
        case 3: if (n > 0) { pw = nullptr; expect_bad = true; } break;
        case 4: if (n > 0) { if (rng() % 2) pin = nullptr; else pout = nullptr; expect_bad = true; } break;
        case 5: nb = rng() % 2 ? 0 : 1025 + (int)(rng() % 5); expect_bad = true; break;       // (refused before any array is read)
        case 6: nn = -1 - (int)(rng() % 5); expect_bad = true; break;
        case 7: if (n > 0) { idx[slot] = rng() % 2 ? nbones + (int32_t)(rng() % 3) : -1 - (int32_t)(rng() % 3); expect_bad = true; } break;
        case 8: if (n > 0) { w[slot] = rng() % 2 ? std::numeric_limits<float>::quiet_NaN() : std::numeric_limits<float>::infinity(); expect_bad = true; } break;
        case 9: if (n > 0) { w[slot] = -0.5f; expect_bad = true; } break;
        case 10: if (n > 0) { w[slot] += 0.01f; expect_bad = true; } break;
        case 11: bones[rng() % bones.size()] = rng() % 2 ? std::numeric_limits<float>::quiet_NaN() : -std::numeric_limits<float>::infinity(); expect_bad = true; break;
        case 12: if (n > 0 && !translations) { for (int b = 0; b < nbones; b++) bones[12 * (size_t)b] = 3.0e38f; for (int v = 0; v < n; v++) in[3 * (size_t)v] = 8.0f; expect_bad = true; } break;
        default: break;
        }
        const int rc = evplp_skin_points(pb, nb, pi, pw, pin, pout, nn);
        if ((rc < 0) != expect_bad) { std::printf("BAD VERDICT it %d spoil %u rc %d\n", it, spoil, rc); return 1; }
        if (rc < 0) {
            if (rc != EVPLP_ERR_INVALID) { std::puts("BAD CODE"); return 1; }
            for (float v : out) if (v != -77.0f) { std::puts("A REFUSAL WROTE"); return 1; }
            bad++; continue;
        }
        ok++;
        for (int v = 0; v < n; v++) for (int r = 0; r < 3; r++) {
            const float got = out[3 * (size_t)v + r];
            if (!std::isfinite(got)) { std::puts("BAD POINT"); return 1; }
            if (translations && got != in[3 * (size_t)v + r] + bones[12 * (size_t)idx[4 * (size_t)v] + 4 * r + 3]) { std::puts("BAD TRANSLATION"); return 1; }
        }
        // in place: the same points
        std::vector<float> again(in);
        if (evplp_skin_points(pb, nb, pi, pw, again.data(), again.data(), nn) != EVPLP_OK || (n > 0 && std::memcmp(again.data(), out.data(), sizeof(float) * out.size()) != 0)) { std::puts("BAD IN PLACE"); return 1; }
    }
    std::printf("skinned %ld refused %ld\n", ok, bad);
    return 0;
}
