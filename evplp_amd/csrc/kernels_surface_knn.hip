// k-nearest-photon start radii for the progressive surface gather (evplp_gather_surface_knn, evplp_bake_lightmap_knn_device;
// surface_gather.cpp, lightmap.cpp).  The grid build and the compact records are kernels_surface.hip's and kernels_surface_prog.hip's,
// launched as they are (launch_surface_grid, launch_surface_prog_compact); this unit owns the two kernels behind them:
//   surface_knn_select_kernel <- lane = point, one wave per workgroup (surface_photon_kernel's comment gives the reason).  For a state with
//                                pm_calls == 0 on a valid finite point and eye: the exact k-th smallest d2 among the photons within the
//                                call's radius r0, by knn_select.h's radix select over d2's bit pattern -- up to eight passes of four bits,
//                                each one walk of the lane's cells as surface_prog_photon_kernel walks them, reading c[4] and c[0] of a
//                                compact record (32 of its 80 bytes).  A pass counts into the lane's own column of uint32 hist[16][64] in
//                                LDS (4 KB): the column is private, so there is no barrier and no atomic, and bin * 64 + lane is free of
//                                bank conflicts whatever the bins; 16 counters indexed at run time would otherwise go to scratch.  Pass 0
//                                also yields C, the photons within r0: a lane with C < k is done and takes r0sq.  A lane whose prefix
//                                already bounds the k-th by rminsq is done too and takes rminsq.  rk2[lane] = min(max(kth, rminsq), r0sq).
//   surface_knn_photon_kernel <- lane = point: surface_prog_photon_kernel's visiting loop with rk2[lane] in the inside test, then ss_seed
//                                (surface_state.h) and the three float4 back.  Which lanes are written is decided as the select decided it;
//                                a point or eye that is not finite is flagged here.
// The unit carries its own copy of the fragment's receiver side (kernels_surface_prog.hip's, operation for operation) and is built without
// contraction: d2 has evo_photon_frag's roundings in both kernels, and the state's rule is the host's, bit for bit.  No atomics, no scratch.
#include "device_common.hpp"
#include "kernels.h"
#include "knn_select.h"
#include "photon_grid.h"
#include "surface_gather.hpp"
#include "surface_state.h"

namespace evplp {

namespace {
EV_DEV bool sk_finite(float x) { return fabsf(x) <= 3.4028235e38f; }        // (false for a NaN)
EV_DEV bool sk_finite(V3 x) { return sk_finite(x.x) && sk_finite(x.y) && sk_finite(x.z); }
EV_DEV V3 sk_eye(const SurfaceProgArgs &a, uint32_t i) {
    if (!a.eyes) return v3(a.fp.camera_pos);
    const float *e = a.eyes + 3 * (size_t)i;
    return v3(e[0], e[1], e[2]);
}
// the fragment shader's helpers (photonsplatinstanced.frag:42-98), as kernels_surface_prog.hip has them
EV_DEV float sk_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
EV_DEV float sk_pow(float d, float e) { return e == 0.0f ? 1.0f : __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(d)); }
EV_DEV V3 sk_lambert_eval(V3 w10, V3 w12, V3 n, V3 rd) {
    if (dot(w10, n) <= 0.0f || dot(w12, n) <= 0.0f) return v3(0.f, 0.f, 0.f);
    return rd * EV_INV_PI;
}
EV_DEV V3 sk_phong_eval(V3 outv, V3 inv_, V3 n, V3 rs, float e) {
    const V3 r = reflect(-inv_, n);
    const float d = dot(outv, r);
    if (d <= 0.00001f) return v3(0.f, 0.f, 0.f);
    return rs * (e + 2.0f) * sk_pow(d, e) * EV_INV_PI * 0.5f;
}
// the words of a state that decide whether this call is the state's: pm_calls == 0 and EVPLP_STATE_INVALID clear
EV_DEV bool sk_fresh(const float4 &q2) { return __float_as_uint(q2.z) == 0u && (__float_as_uint(q2.w) & EVPLP_STATE_INVALID) == 0u; }
}

__global__ __launch_bounds__(64) void surface_knn_select_kernel(SurfaceKnnArgs a) {
    __shared__ uint32_t hist[16 * 64];                                      // [bin][lane]: a lane reads and writes its own column only
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + lane;
    if (i >= (uint32_t)a.p.n) return;
    const float4 gp = a.p.points[4 * (size_t)i];
    if (gp.w == 0.0f) return;                                               // the stencil
    if (!sk_fresh(a.p.states[3 * (size_t)i + 2])) return;                   // not this call's
    const V3 X = v3(gp);
    if (!sk_finite(X) || !sk_finite(sk_eye(a.p, i))) return;                // (the photon kernel flags it)
    const float r0sq = a.p.r0sq;
    float rk2 = r0sq;
    const float xs[3] = { X.x, X.y, X.z };
    int32_t c0[3], c1[3];
    // (one farther than r0's reach from the scene's box: C = 0 without touching the table)
    if (pg_range(xs, a.p.grid.radius, a.p.grid.lo, a.p.grid.hi, a.p.grid.edge, c0, c1)) {
        for (int k = 0; k < 3; k++) c1[k] = min(c1[k], c0[k] + 2);
        const uint32_t rmin_bits = __float_as_uint(a.rminsq);
        uint32_t prefix = 0u, left = a.k;
        for (uint32_t pass = 0u; pass < KS_PASSES; pass++) {
            for (uint32_t d = 0u; d < 16u; d++) hist[d * 64u + lane] = 0u;
            for (int32_t cz = c0[2]; cz <= c1[2]; cz++) for (int32_t cy = c0[1]; cy <= c1[1]; cy++) for (int32_t cx = c0[0]; cx <= c1[0]; cx++) {
                const uint32_t bk = pg_bucket(cx, cy, cz, a.p.grid.bits);
                const uint32_t jb = a.p.grid.start[bk], je = a.p.grid.start[bk + 1u];
                for (uint32_t j = jb; j < je; j++) {
                    const float4 *c = a.p.grid.compact + (size_t)j * kSurfaceCompactF4;
                    const float4 c4 = c[4];
                    if (__float_as_int(c4.x) != cx || __float_as_int(c4.y) != cy || __float_as_int(c4.z) != cz) continue;       // this cell's photons only
                    const V3 dv = v3(c[0]) - X;
                    const float d2 = dot_exact(dv, dv);                     // evo_photon_frag's roundings
                    if (d2 > r0sq) continue;                                // not a candidate
                    const uint32_t bits = __float_as_uint(d2);
                    if (ks_match(bits, prefix, pass)) hist[ks_digit(bits, pass) * 64u + lane]++;
                }
            }
            uint32_t h[16];
            for (uint32_t d = 0u; d < 16u; d++) h[d] = hist[d * 64u + lane];
            if (pass == 0u) {
                uint32_t C = 0u;
                for (uint32_t d = 0u; d < 16u; d++) C += h[d];
                if (C < left) break;                                        // fewer than k within r0: r0sq
            }
            prefix = (prefix << 4) | ks_step(h, &left);
            if (pass + 1u == KS_PASSES) rk2 = ks_clamp(__uint_as_float(prefix), a.rminsq, r0sq);
            else if (ks_prefix_max(prefix, pass) <= rmin_bits) { rk2 = a.rminsq; break; }      // kth <= rminsq whatever the lower digits
        }
    }
    a.rk2[i] = rk2;
}

__global__ __launch_bounds__(64) void surface_knn_photon_kernel(SurfaceKnnArgs a) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= (uint32_t)a.p.n) return;
    const float4 *pt = a.p.points + 4 * (size_t)i;
    const float4 gp = pt[0];
    if (gp.w == 0.0f) return;                                               // the stencil: not touched at all
    float4 *s = a.p.states + 3 * (size_t)i;
    const float4 sq2 = s[2];
    if (!sk_fresh(sq2)) return;                                             // a state that has been through a photon half, or a flagged one: not a byte
    const V3 eye = sk_eye(a.p, i);
    const V3 X = v3(gp);
    // (a flagged state keeps every other byte: one word is written)
    if (!sk_finite(X) || !sk_finite(eye)) { reinterpret_cast<uint32_t *>(s)[11] = __float_as_uint(sq2.w) | EVPLP_STATE_INVALID; return; }
    const float4 sq0 = s[0], sq1 = s[1];
    evplp_surface_state st;
    st.tau[0] = sq0.x; st.tau[1] = sq0.y; st.tau[2] = sq0.z; st.radius2 = sq0.w;
    st.vpl[0] = sq1.x; st.vpl[1] = sq1.y; st.vpl[2] = sq1.z; st.n = sq1.w;
    st.lit_sum = sq2.x; st.vpl_calls = __float_as_uint(sq2.y); st.pm_calls = 0u; st.flags = __float_as_uint(sq2.w);
    const float r2 = a.rk2[i];                                              // the select's: within [rminsq, r0sq]
    const float xs[3] = { X.x, X.y, X.z };
    int32_t c0[3], c1[3];
    V3 sum = v3(0.f, 0.f, 0.f);
    uint32_t pairs = 0u;
    if (pg_range(xs, ss_radius_bound(r2, a.p.grid.radius), a.p.grid.lo, a.p.grid.hi, a.p.grid.edge, c0, c1)) {
        const float4 gn = pt[1], gd = pt[2], gs = pt[3];
        const V3 sn = v3(gn), sd = v3(gd), sps = v3(gs); const float se = gs.w;
        const V3 w10 = normalize(eye - X);                                  // frag:177
        const uint32_t mode = a.p.fp.mis_mode;
        const float clampv = a.p.fp.clamping_value;
        const bool glossy = sps.x != 0.0f || sps.y != 0.0f || sps.z != 0.0f;
        for (int k = 0; k < 3; k++) c1[k] = min(c1[k], c0[k] + 2);
        for (int32_t cz = c0[2]; cz <= c1[2]; cz++) for (int32_t cy = c0[1]; cy <= c1[1]; cy++) for (int32_t cx = c0[0]; cx <= c1[0]; cx++) {
            const uint32_t bk = pg_bucket(cx, cy, cz, a.p.grid.bits);
            const uint32_t jb = a.p.grid.start[bk], je = a.p.grid.start[bk + 1u];
            for (uint32_t j = jb; j < je; j++) {
                const float4 *c = a.p.grid.compact + (size_t)j * kSurfaceCompactF4;
                const float4 c4 = c[4];
                if (__float_as_int(c4.x) != cx || __float_as_int(c4.y) != cy || __float_as_int(c4.z) != cz) continue;       // this cell's photons only
                const float4 q0 = c[0];
                const V3 dv = v3(q0) - X;
                if (dot_exact(dv, dv) > r2) continue;                       // evo_photon_frag's roundings, the lane's selected radius2
                pairs++;
                const float4 q1 = c[1], q2 = c[2];
                const V3 w12 = v3(q1);
                V3 brdf1 = sk_lambert_eval(w10, w12, sn, sd);               // frag:181
                if (glossy) brdf1 = brdf1 + sk_phong_eval(w10, w12, sn, sps, se);
                if (q2.w == 0.0f) continue;                                 // mixPdfW > 0, frag:191
                V3 col;
                if (mode == 0u) col = brdf1 * v3(q2);
                else {
                    const float cc = fmaxf(dot(sn, w12), 0.0f) * q0.w;      // frag:216,226
                    if (cc <= 0.0f) continue;                               // discard
                    const float g = cc * sk_rcp(q1.w);
                    if (mode == 4u) col = (brdf1 * v3(q2)) * (fmaxf(g - clampv, 0.0f) * sk_rcp(g));
                    else {
                        const V3 brdf2 = v3(c[3]);
                        V3 num = (brdf1 * brdf2) * g;
                        num = v3(fmaxf(num.x - clampv, 0.f), fmaxf(num.y - clampv, 0.f), fmaxf(num.z - clampv, 0.f));
                        const V3 den = brdf2 * g;
                        const V3 pre = v3(q2);
                        // zero denominator contributes 0 (the reference produces NaN here)
                        col = v3(den.x != 0.f ? pre.x * num.x * sk_rcp(den.x) : 0.f, den.y != 0.f ? pre.y * num.y * sk_rcp(den.y) : 0.f,
                                 den.z != 0.f ? pre.z * num.z * sk_rcp(den.z) : 0.f);
                    }
                }
                sum = sum + col;
            }
        }
    }
    const float phi[3] = { sum.x, sum.y, sum.z };
    ss_seed(&st, r2, pairs, phi, a.p.alpha);
    s[0] = make_float4(st.tau[0], st.tau[1], st.tau[2], st.radius2);
    s[1] = make_float4(sq1.x, sq1.y, sq1.z, st.n);
    s[2] = make_float4(sq2.x, sq2.y, __uint_as_float(st.pm_calls), sq2.w);
}

void launch_surface_knn_select(const SurfaceKnnArgs &a, hipStream_t s) {
    if (a.p.n <= 0) return;
    hipLaunchKernelGGL(surface_knn_select_kernel, dim3((uint32_t)(((int64_t)a.p.n + 63) / 64)), dim3(64), 0, s, a);
}
void launch_surface_knn_photons(const SurfaceKnnArgs &a, hipStream_t s) {
    if (a.p.n <= 0) return;
    hipLaunchKernelGGL(surface_knn_photon_kernel, dim3((uint32_t)(((int64_t)a.p.n + 63) / 64)), dim3(64), 0, s, a);
}

} // namespace evplp
