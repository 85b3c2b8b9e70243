// The noise tracker's per-pixel arithmetic, shared by kernels_trace.hip (the estimate, the variance image, evplp_adaptive_retire) and
// kernels_ptbatch_primary.hip (evplp_adaptive_tile_noise).  Both units are built without contraction and every operation is an _rn intrinsic.
#pragma once
#include "device_common.hpp"
#include "kernels.h"

namespace evplp {

// Q and S of pixel i, per channel
__device__ inline void noise_moments(const NoiseMoments &m, size_t i, double q[3], double s[3]) {
    for (int ch = 0; ch < 3; ch++) q[ch] = m.q[ch * m.stride + i];
    if (m.s) { for (int ch = 0; ch < 3; ch++) s[ch] = m.s[ch * m.stride + i]; return; }
    const float4 a = m.prev[i], b = m.start[i];
    s[0] = (double)__fsub_rn(a.x, b.x); s[1] = (double)__fsub_rn(a.y, b.y); s[2] = (double)__fsub_rn(a.z, b.z);
}
// the variance of one channel of the image scale * c: s2K * max(0, (Q - S * S / K) / (B - 1)), s2K = scale^2 * K
__device__ inline double noise_var(double q, double s, double K, double B1, double s2K) {
    const double v = __ddiv_rn(__dsub_rn(q, __ddiv_rn(__dmul_rn(s, s), K)), B1);
    return __dmul_rn(s2K, v > 0.0 ? v : 0.0);
}
// the variance of one channel of a RETIRED pixel (tile record r): the tracker's figure at retirement, rescaled to today's composite --
// noise_var(Q, S, K_t, B_t - 1, s2K_t), s2K_t = ((scale * N) / n_t)^2 * K_t
__device__ inline double noise_var_retired(double q, double s, const int4 &r, const AdaptTiles &at) {
    const double f = __ddiv_rn(__dmul_rn(at.scale, at.n), (double)r.x);
    return noise_var(q, s, (double)r.y, (double)r.z - 1.0, __dmul_rn(__dmul_rn(f, f), (double)r.y));
}
// num of pixel i (tile record at ty * tiles_x + tx, Adapt only) from its moments: (var_r + var_g) + var_b, fp64
template <bool Adapt>
__device__ inline double noise_num(const double q[3], const double sm[3], double K, double B1, double s2K, const AdaptTiles &at, int l, int x) {
    if constexpr (Adapt) {
        const int4 r = at.tiles[(l >> 3) * at.tiles_x + (x >> 3)];
        if (r.x != 0) return __dadd_rn(__dadd_rn(noise_var_retired(q[0], sm[0], r, at), noise_var_retired(q[1], sm[1], r, at)), noise_var_retired(q[2], sm[2], r, at));
    }
    return __dadd_rn(__dadd_rn(noise_var(q[0], sm[0], K, B1, s2K), noise_var(q[1], sm[1], K, B1, s2K)), noise_var(q[2], sm[2], K, B1, s2K));
}
// A tile's rel, summed: lane = pixel (x, local row l).  The lane forms noise_rows_kernel's rel (0 outside the image); the sum over the 64
// lanes is a fixed tree (shuffle-down by 32, 16, .. 1) and so is the count of in-image pixels; every lane returns lane 0's pair.
template <bool Adapt>
__device__ __forceinline__ void tile_rel_sum(const StripDev &st, const NoiseMoments &m, double K, double B1, double s2K, const float4 *light, float ls,
                                             int mask_emitter, const float *rgb, const AdaptTiles &at, int x, int l, double &rel, double &cnt) {
    const bool in = x < st.W && l < st.local_rows && st.global_row(l) < st.H;
    rel = 0.0; cnt = in ? 1.0 : 0.0;
    if (in) {
        const size_t i = (size_t)l * st.W + x;
        double num = 0.0;
        if (!(mask_emitter && 0.0f < __fmul_rn(light[i].x, ls))) {
            double q[3], sm[3];
            noise_moments(m, i, q, sm);
            num = noise_num<Adapt>(q, sm, K, B1, s2K, at, l, x);
        }
        const double r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        rel = __ddiv_rn(num, __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(r, r), __dmul_rn(g, g)), __dmul_rn(b, b)), 0.001));
    }
    for (int off = 32; off > 0; off >>= 1) { rel = __dadd_rn(rel, __shfl_down(rel, off, 64)); cnt = __dadd_rn(cnt, __shfl_down(cnt, off, 64)); }
    rel = __shfl(rel, 0, 64); cnt = __shfl(cnt, 0, 64);
}

} // namespace evplp
