/*
 * knn_select.h -- the exact select behind the k-nearest-photon start radius of the progressive surface gather (evplp_gather_surface_knn,
 * include/evplp.h), written once for the host (host/knn_select.cpp exports it as evplp_knn_radius2) and for surface_knn_select_kernel
 * of kernels_surface_knn.hip, as photon_grid.h is for the grid.  Integer operations, two comparisons and fminf / fmaxf: nothing rounds.
 *
 * What is selected.  The candidates of a point are the photons whose d2 -- evo_photon_frag's (dv.x dv.x + dv.y dv.y) + dv.z dv.z, every
 * operation rounded on its own -- passes !(d2 > r0sq).  Such a d2 is a sum of squares: never negative, never -0, and (below) never a NaN,
 * so bit 31 of its pattern is clear and two of them order as their patterns do as uint32.  The k-th smallest, with multiplicity, is
 * therefore the k-th smallest pattern, and a most-significant-digit radix select finds it without comparing floats: eight passes of four
 * bits from the top; a pass counts, per value of its digit, the candidates whose higher digits equal the prefix chosen so far (ks_match),
 * and ks_step picks the digit that holds the k-th and takes the lower digits' count off k.  After eight passes the prefix IS the pattern.
 *
 * No NaN among the candidates.  A d2 is a NaN only where dv has a NaN or dv's squares overflow to inf - inf; X is finite (the kernels
 * flag a point that is not), so that needs a photon coordinate that is a NaN (an infinite one gives d2 = inf, which is outside).
 * pg_cell1 puts a NaN coordinate on cell PG_CELL_MIN = -8 of its axis.  A walked point -- pg_range returned 1 -- has
 * fl(x + reach) >= lo on every axis, so fl(x - reach) lies less than one edge below lo (photon_grid.h's edge argument: the two ends
 * differ by at most 2 reach + 2^-21 M < edge): the low end of its range is cell -1 at the least.  The own-cell test of the walk (c[4] against the visited cell) therefore never lets such a photon through,
 * whatever bucket it hashes to.  evplp_knn_radius2, which has no grid in front of it, refuses an array that holds a NaN or a set bit 31.
 */
#ifndef EVPLP_KNN_SELECT_H
#define EVPLP_KNN_SELECT_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KS_FN __host__ __device__ static inline
#else
#define KS_FN static inline
#endif

#define KS_PASSES 8u        /* of four bits each, from the top */

/* the digit of pass 0 .. 7: bits 31-28, 27-24, ... 3-0 (pass 0 sees 0 .. 7: bit 31 is clear) */
KS_FN uint32_t ks_digit(uint32_t bits, uint32_t pass) { return (bits >> (28u - 4u * pass)) & 15u; }

/* 1: the digits above pass `pass` of bits are the prefix chosen in passes 0 .. pass - 1 (always, in pass 0) */
KS_FN int ks_match(uint32_t bits, uint32_t prefix, uint32_t pass) { return pass == 0u || (bits >> (32u - 4u * pass)) == prefix; }

/* The smallest digit whose cumulative count reaches *k_remaining; the lower digits' count is taken off *k_remaining, which then counts
 * within that digit.  The caller has made sure that the 16 counts sum to *k_remaining at the least.  (No early exit: with constant
 * indices the 16 counts stay in registers.) */
KS_FN uint32_t ks_step(const uint32_t hist[16], uint32_t *k_remaining) {
    const uint32_t k = *k_remaining;
    uint32_t below = 0u, digit = 15u, taken = 0u;
    int found = 0;
    for (uint32_t d = 0u; d < 16u; d++) {
        const uint32_t upto = below + hist[d];
        if (!found && upto >= k) { digit = d; taken = below; found = 1; }
        below = upto;
    }
    *k_remaining = k - taken;
    return digit;
}

/* Every pattern that starts with `prefix` after passes 0 .. pass is at most this one. */
KS_FN uint32_t ks_prefix_max(uint32_t prefix, uint32_t pass) {
    const uint32_t low = 28u - 4u * pass;
    return (prefix << low) | ((1u << low) - 1u);
}

/* rk2 = min(max(kth, rminsq), r0sq) */
KS_FN float ks_clamp(float kth, float rminsq, float r0sq) { return fminf(fmaxf(kth, rminsq), r0sq); }

#endif /* EVPLP_KNN_SELECT_H */
