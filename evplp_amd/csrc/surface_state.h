/*
 * surface_state.h -- the per-point state of the progressive surface gather (evplp_gather_surface_progressive, include/evplp.h) and its
 * rule, written once for the host (host/surface_state.cpp exports it as evplp_surface_state_update / _resolve) and for the kernels of
 * kernels_surface_prog.hip, as photon_grid.h is for the grid.  Only + - * / comparisons and integer operations, none contracted: every
 * operation is rounded to fp32 on its own and a division is IEEE's, so n and radius2 can be restated bit for bit.
 *
 * The rule is stochastic progressive photon mapping's (Hachisuka and Jensen 2009) with the radius kept squared.  One call found M photons
 * within radius2 of the point, of unnormalised flux phi (the fragment's value without InvPi / r^2):
 *     Nn = n + alpha M,  ratio = Nn / (n + M),  radius2 *= ratio,  tau = (tau + phi) ratio,  n = Nn            (M > 0; else nothing)
 * alpha <= 1 and monotone rounding give fl(n + fl(alpha M)) <= fl(n + M), hence ratio <= 1: a radius never grows, and radius2 <= r0sq, the
 * square of the call's bound, holds for every state the rule itself has made.
 *
 * The range.  photon_grid.h proves, for the test d2 > fl(r r) and reach = max(fl(r (1 + 2^-20)), 2^-59), the inclusion
 * fl(X - reach) <= P <= fl(X + reach) for every photon the test calls inside, and a range at most two cells wide for an edge
 * >= 2 reach (1 + 2^-4).  Here the test is d2 > radius2 with the point's own radius2 <= r0sq = fl(r0 r0) on the grid planned for r0.
 *   The inclusion with the call's bound.  An inside photon has each fl(dv_k dv_k) <= radius2 <= fl(r0 r0): the header's argument word for
 *     word, so pg_range(x, r0, ...) is always valid -- the fallback.
 *   The inclusion with a smaller bound.  Let s be an fp32 number with fl(s s) >= radius2 and radius2 >= 2^-100 (the product is normal).
 *     Then s^2 >= radius2 (1 - 2^-24), s >= sqrt(radius2) (1 - 2^-24), and an inside photon's true |P_k - X_k| <= sqrt(radius2) (1 + 2^-22)
 *     <= s (1 + 2^-22) (1 + 2^-23) < fl(s (1 + 2^-20)): pg_range(x, s, ...) pads s exactly as it pads a radius, and its inclusion holds.
 *     ss_radius_bound makes such an s without a square root: the float whose bits are (bits(radius2) >> 1) + 0x1fc00000 is 2^k (1 + f / 2)
 *     for radius2 = 2^2k (1 + f) and 2^k (1.5 + f / 2) for 2^(2k+1) (1 + f), never below the root and at most 6.1 % above it -- and the
 *     property the proof needs, fl(s s) >= radius2, is TESTED, not trusted: where it fails (or radius2 < 2^-100) the call's bound is taken.
 *   The width.  The edge was planned for r0: edge >= 2 reach(r0) (1 + 2^-4).  min(s, r0) <= r0 makes the reach no larger, which only
 *     loosens that inequality: the range stays at most two cells per axis.
 */
#ifndef EVPLP_SURFACE_STATE_H
#define EVPLP_SURFACE_STATE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SS_FN __host__ __device__ static inline
#else
#define SS_FN static inline
#endif
#if defined(__clang__)
#define SS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SS_NO_CONTRACT
#endif

#define SS_INV_PI 0.318309886183790671537767526745028724068919291480912897495f      /* EV_INV_PI */

SS_FN int ss_finite(float x) { return fabsf(x) <= 3.4028235e38f; }      /* (false for a NaN) */
SS_FN uint32_t ss_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
SS_FN float ss_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

/* 1: a call that asks for photons may walk this state.  0: it has been through a photon half and its radius2 is not in (0, r0sq] */
SS_FN int ss_radius_ok(uint32_t pm_calls, float radius2, float r0sq) {
    if (pm_calls == 0u) return 1;                                       /* (radius2 = r0sq is still to come) */
    return ss_finite(radius2) && radius2 > 0.0f && radius2 <= r0sq;
}

/* a "radius" for pg_range: an upper bound of sqrt(radius2) in the sense of the note above, never above the call's */
SS_FN float ss_radius_bound(float radius2, float r_call) {
    SS_NO_CONTRACT
    const float s = ss_float((ss_bits(radius2) >> 1) + 0x1fc00000u);
    if (!(radius2 >= 0x1p-100f) || !(s * s >= radius2)) return r_call;
    return fminf(s, r_call);
}

/* one photon half of one point: M photons inside, phi their summed value.  The caller has looked at ss_radius_ok. */
SS_FN void ss_update(evplp_surface_state *st, uint32_t M, const float phi[3], float alpha, float r0sq) {
    SS_NO_CONTRACT
    if (st->pm_calls == 0u) st->radius2 = r0sq;
    if (M > 0u) {
        const float m = (float)M;
        const float nn = st->n + alpha * m;
        const float ratio = nn / (st->n + m);
        st->radius2 = st->radius2 * ratio;
        for (int k = 0; k < 3; k++) st->tau[k] = (st->tau[k] + phi[k]) * ratio;
        st->n = nn;
    }
    st->pm_calls++;
}

/* the first photon half of a state with pm_calls == 0 at a radius2 chosen for the point (evplp_gather_surface_knn: the k-th nearest
 * photon's d2, clamped into [rminsq, r0sq]) instead of r0sq: M photons inside it, phi their summed value.  ss_update's M > 0 branch. */
SS_FN void ss_seed(evplp_surface_state *st, float radius2, uint32_t M, const float phi[3], float alpha) {
    SS_NO_CONTRACT
    st->radius2 = radius2;
    if (M > 0u) {
        const float m = (float)M;
        const float nn = st->n + alpha * m;
        const float ratio = nn / (st->n + m);
        st->radius2 = st->radius2 * ratio;
        for (int k = 0; k < 3; k++) st->tau[k] = (st->tau[k] + phi[k]) * ratio;
        st->n = nn;
    }
    st->pm_calls = 1u;
}

SS_FN void ss_resolve(const evplp_surface_state *st, evplp_surface_light *out) {
    SS_NO_CONTRACT
    for (int k = 0; k < 3; k++) { out->vpl[k] = 0.0f; out->pm[k] = 0.0f; }
    out->lit = 0.0f; out->photons = 0.0f;
    if (st->flags & EVPLP_STATE_INVALID) { out->lit = -1.0f; out->photons = -1.0f; return; }
    if (st->vpl_calls > 0u) {
        const float d = (float)st->vpl_calls;
        for (int k = 0; k < 3; k++) out->vpl[k] = st->vpl[k] / d;
        out->lit = st->lit_sum / d;
    }
    if (st->pm_calls > 0u) {
        const float d = st->radius2 * (float)st->pm_calls;
        for (int k = 0; k < 3; k++) out->pm[k] = (st->tau[k] * SS_INV_PI) / d;
        out->photons = st->n;
    }
}

#endif /* EVPLP_SURFACE_STATE_H */
