// k-nearest-photon start radii, host only (include/evplp.h "k-nearest-photon start radii"): the radix select over an array of d2 values
// and the seeding of one state, exported from the headers the kernels of kernels_surface_knn.hip include (knn_select.h,
// surface_state.h).  No GPU, no context: the tests hold the select against a sort and the seed against a numpy float32 restatement, bit
// for bit, with these.
#include "../../../include/evplp.h"
#include "../knn_select.h"
#include "../surface_state.h"

extern "C" int evplp_knn_radius2(const float *d2, uint32_t count, uint32_t k, float rminsq, float r0sq, float *radius2, uint32_t *m) {
    if ((!d2 && count > 0u) || !radius2 || !m || k == 0u) return EVPLP_ERR_INVALID;
    if (!ss_finite(rminsq) || !ss_finite(r0sq) || !(rminsq > 0.0f) || rminsq > r0sq) return EVPLP_ERR_INVALID;
    for (uint32_t i = 0; i < count; i++) if (d2[i] != d2[i] || (ss_bits(d2[i]) >> 31)) return EVPLP_ERR_INVALID;
    float rk2 = r0sq;
    uint32_t prefix = 0u, left = k;
    // the kernel's passes, an array in the place of the walk
    for (uint32_t pass = 0u; pass < KS_PASSES; pass++) {
        uint32_t hist[16] = { 0u };
        for (uint32_t i = 0; i < count; i++) {
            if (d2[i] > r0sq) continue;                                     // not a candidate
            const uint32_t bits = ss_bits(d2[i]);
            if (ks_match(bits, prefix, pass)) hist[ks_digit(bits, pass)]++;
        }
        if (pass == 0u) {
            uint32_t C = 0u;
            for (uint32_t d = 0u; d < 16u; d++) C += hist[d];
            if (C < left) break;                                            // fewer than k candidates: r0sq
        }
        prefix = (prefix << 4) | ks_step(hist, &left);
        if (pass + 1u == KS_PASSES) rk2 = ks_clamp(ss_float(prefix), rminsq, r0sq);
        else if (ks_prefix_max(prefix, pass) <= ss_bits(rminsq)) { rk2 = rminsq; break; }
    }
    uint32_t inside = 0u;
    for (uint32_t i = 0; i < count; i++) if (!(d2[i] > r0sq) && !(d2[i] > rk2)) inside++;
    *radius2 = rk2; *m = inside;
    return EVPLP_OK;
}

extern "C" int evplp_surface_state_seed(evplp_surface_state *state, float radius2, uint32_t m, const float phi[3], float alpha, float r0sq) {
    if (!state || !phi) return EVPLP_ERR_INVALID;
    if (state->pm_calls > 0u || (state->flags & EVPLP_STATE_INVALID)) return EVPLP_ERR_INVALID;
    if (!ss_finite(radius2) || !(radius2 > 0.0f) || !(radius2 <= r0sq)) return EVPLP_ERR_INVALID;
    ss_seed(state, radius2, m, phi, alpha);
    return EVPLP_OK;
}
