/*
 * photon_grid.h -- the world-space grid of the surface gather's photon half (evplp_gather_surface), written once for the host
 * (host/photon_grid.cpp exports it as evplp_photon_grid_plan / _cell / _range) and for the kernels of kernels_surface.hip, as ev_math.h
 * is for the samplers.  Only + - * / floorf fminf fmaxf and integer operations, none contracted.
 *
 * The test the grid serves is evo_photon_frag's: dv = P - X per component, d2 = (dv.x dv.x + dv.y dv.y) + dv.z dv.z, every operation
 * rounded to fp32 on its own, and the photon is outside iff d2 > r r (r r rounded too).  The grid may only be conservative about it.
 *
 * The pad (include/evplp.h states the same argument).  Let the test say inside.  Sums of non-negative terms round monotonically, so each
 * fl(dv_k dv_k) <= fl(r r) <= r^2 (1 + 2^-24); with s = |fl(P_k - X_k)| and a normal product, s^2 (1 - 2^-24) <= r^2 (1 + 2^-24), i.e.
 * s <= r (1 + 2^-23).  (A product that underflows has s < 2^-60.)  The subtraction errs by at most 2^-24 relative, never absolutely, so
 * the true |P_k - X_k| <= max(r (1 + 2^-22), 2^-59).  reach = max(fl(r (1 + 2^-20)), 2^-59) exceeds that, and because P_k is an fp32
 * number and rounding is monotone,   fl(X_k - reach) <= P_k <= fl(X_k + reach).
 * The cell of a coordinate, cell(p) = floor(clamp(fl(fl(p - lo) / edge), -8, 2^17)), is a composition of monotone functions, so
 *     cell(fl(X_k - reach)) <= cell(P_k) <= cell(fl(X_k + reach))
 * whatever the subtraction and the division round to: the rounding of (x +- r - lo) / edge cannot lose a photon, it is the same function
 * on both sides.  That is the whole correctness argument; the edge only decides how many cells the range spans.
 * The edge.  With every magnitude |X_k| + reach and |a - lo| at most M, the two ends of the range differ, after the four roundings, by
 * at most (2 reach + 2^-21 M) / edge.  edge = max(2 reach (1 + 2^-4), 2^-16 M) makes that 1 / 1.0625 + 2^-5 < 1: a walked point's range
 * is at most 2 cells per axis (the tests hold it to the 3 the interface promises), and cell indices stay within [-8, 2^17].
 * M = max |lo_k|, |hi_k| over the axes + the largest extent + 4 reach bounds every walked point: one farther than reach from the box on
 * some axis is not walked at all (evplp_photon_grid_range returns 0).
 */
#ifndef EVPLP_PHOTON_GRID_H
#define EVPLP_PHOTON_GRID_H

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FN __host__ __device__ static inline
#else
#define PG_FN static inline
#endif
#if defined(__clang__)
#define PG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define PG_NO_CONTRACT
#endif

#define PG_MIN_BITS 4u
#define PG_MAX_BITS 24u
#define PG_CELL_MIN (-8.0f)
#define PG_CELL_MAX 131072.0f

PG_FN int pg_finite(float x) { return fabsf(x) <= 3.4028235e38f; }      /* (false for a NaN) */

PG_FN float pg_reach(float radius) {
    PG_NO_CONTRACT
    return fmaxf(radius * (1.0f + 0x1p-20f), 0x1p-59f);
}

/* 1 and *edge, *bits; 0 for a radius that is not positive and finite, a box that is not finite or has lo > hi, an edge that overflows */
PG_FN int pg_plan(float radius, const float lo[3], const float hi[3], uint32_t usable, float *edge, uint32_t *bits) {
    PG_NO_CONTRACT
    if (!pg_finite(radius) || !(radius > 0.0f)) return 0;
    const float reach = pg_reach(radius);
    float mag = 0.0f, ext = 0.0f;
    for (int k = 0; k < 3; k++) {
        if (!pg_finite(lo[k]) || !pg_finite(hi[k]) || lo[k] > hi[k]) return 0;
        mag = fmaxf(mag, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
        ext = fmaxf(ext, hi[k] - lo[k]);
    }
    const float m = (mag + ext) + 4.0f * reach;
    const float e = fmaxf((2.0f * reach) * (1.0f + 0x1p-4f), m * 0x1p-16f);
    if (!pg_finite(e) || !pg_finite(m)) return 0;
    uint32_t b = PG_MIN_BITS;
    while (b < PG_MAX_BITS && (1u << b) < usable) b++;
    *edge = e; *bits = b;
    return 1;
}

PG_FN int32_t pg_cell1(float p, float lo, float edge) {
    PG_NO_CONTRACT
    const float u = p - lo;
    const float t = u / edge;
    return (int32_t)floorf(fminf(fmaxf(t, PG_CELL_MIN), PG_CELL_MAX));      /* (a NaN lands on PG_CELL_MIN) */
}

/* the cells [c0, c1] per axis that hold every photon the fp32 test can call inside; 0: the point is farther than the reach from the
 * box on some axis and no photon inside the box can pass */
PG_FN int pg_range(const float x[3], float radius, const float lo[3], const float hi[3], float edge, int32_t c0[3], int32_t c1[3]) {
    PG_NO_CONTRACT
    const float reach = pg_reach(radius);
    int walk = 1;
    for (int k = 0; k < 3; k++) {
        const float a = x[k] - reach, b = x[k] + reach;
        if (b < lo[k] || a > hi[k]) walk = 0;
        c0[k] = pg_cell1(a, lo[k], edge); c1[k] = pg_cell1(b, lo[k], edge);
    }
    return walk;
}

/* the bucket of a cell among 2^bits (Teschner et al. 2003, then a finaliser so that the low bits see every axis) */
PG_FN uint32_t pg_bucket(int32_t cx, int32_t cy, int32_t cz, uint32_t bits) {
    uint32_t h = ((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u);
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h & ((1u << bits) - 1u);
}

#endif /* EVPLP_PHOTON_GRID_H */
