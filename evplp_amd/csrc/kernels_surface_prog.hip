// Progressive surface gather (evplp_gather_surface_progressive, evplp_surface_resolve, evplp_bake_lightmap_resolve; surface_gather.cpp,
// lightmap.cpp): per-point photon statistics with per-point radii.  The VPL half and the grid build are kernels_surface.hip's, launched as
// they are; this unit owns what the per-point state needs:
//   surface_prog_compact_kernel  <- behind the grid build: the compact records' wflux again, as flux * rcp((float)num_light_paths) -- InvPi *
//                                   uInvPhotonRadius2 taken out, the weight 1 (mis_mode 0, 4, 5); every other field stays surface_compact_kernel's
//   surface_prog_fold_kernel     <- lane = point: the 16 bytes surface_reduce_kernel wrote for the point, added into the state's running sums
//   surface_prog_photon_kernel   <- lane = point, one wave per workgroup (surface_photon_kernel's comment gives the reason): the state's
//                                   three float4, the range of the LANE's radius (surface_state.h), surface_photon_kernel's visiting loop
//                                   with the lane's radius2 in the inside test, the update of surface_state.h, the three float4 back.  Loop
//                                   bounds and bucket loads are per lane: lanes of one wave have different ranges and trip counts.
//   surface_prog_resolve_kernel  <- lane = state: surface_state.h's resolve
//   lightmap_prog_resolve_kernel <- lane = texel: its samples' resolved states in ascending (j, i), the mean, the coverage
// The unit carries its own copy of the fragment's receiver side (kernels_surface.hip's, operation for operation) and is built without
// contraction: the inside test has evo_photon_frag's roundings and the state's rule is the host's, bit for bit.  No float atomics, no scratch.
#include "device_common.hpp"
#include "kernels.h"
#include "photon_grid.h"
#include "surface_gather.hpp"
#include "surface_state.h"

namespace evplp {

namespace {
EV_DEV bool sp_finite(float x) { return fabsf(x) <= 3.4028235e38f; }        // (false for a NaN)
EV_DEV bool sp_finite(V3 x) { return sp_finite(x.x) && sp_finite(x.y) && sp_finite(x.z); }
EV_DEV V3 sp_eye(const SurfaceProgArgs &a, uint32_t i) {
    if (!a.eyes) return v3(a.fp.camera_pos);
    const float *e = a.eyes + 3 * (size_t)i;
    return v3(e[0], e[1], e[2]);
}
// the fragment shader's helpers (photonsplatinstanced.frag:42-98), as kernels_surface.hip has them
EV_DEV float sp_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
EV_DEV float sp_pow(float d, float e) { return e == 0.0f ? 1.0f : __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(d)); }
EV_DEV V3 sp_lambert_eval(V3 w10, V3 w12, V3 n, V3 rd) {
    if (dot(w10, n) <= 0.0f || dot(w12, n) <= 0.0f) return v3(0.f, 0.f, 0.f);
    return rd * EV_INV_PI;
}
EV_DEV V3 sp_phong_eval(V3 outv, V3 inv_, V3 n, V3 rs, float e) {
    const V3 r = reflect(-inv_, n);
    const float d = dot(outv, r);
    if (d <= 0.00001f) return v3(0.f, 0.f, 0.f);
    return rs * (e + 2.0f) * sp_pow(d, e) * EV_INV_PI * 0.5f;
}
// the state as its three float4
struct SpState { float4 q0, q1, q2; };
EV_DEV SpState sp_load(const float4 *states, size_t i) { const float4 *s = states + 3 * i; SpState r; r.q0 = s[0]; r.q1 = s[1]; r.q2 = s[2]; return r; }
EV_DEV evplp_surface_state sp_unpack(const SpState &s) {
    evplp_surface_state st;
    st.tau[0] = s.q0.x; st.tau[1] = s.q0.y; st.tau[2] = s.q0.z; st.radius2 = s.q0.w;
    st.vpl[0] = s.q1.x; st.vpl[1] = s.q1.y; st.vpl[2] = s.q1.z; st.n = s.q1.w;
    st.lit_sum = s.q2.x; st.vpl_calls = __float_as_uint(s.q2.y); st.pm_calls = __float_as_uint(s.q2.z); st.flags = __float_as_uint(s.q2.w);
    return st;
}
// (a flagged state keeps every other byte: one word is written)
EV_DEV void sp_flag(float4 *states, uint32_t i, uint32_t flags) { reinterpret_cast<uint32_t *>(states + 3 * (size_t)i)[11] = flags | EVPLP_STATE_INVALID; }
}

__global__ __launch_bounds__(256) void surface_prog_compact_kernel(SurfaceGridBuild b) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= b.g.slots) return;
    if (b.keys_sorted[j] >> b.g.bits) return;                               // an unusable slot: nothing reads its record
    const uint32_t i = b.vals_sorted[j];
    const float4 flux = reinterpret_cast<const float4 *>(b.records + i)[2];
    const float inv_n = sp_rcp((float)b.fp.num_light_paths);                // uInvNumLightPaths
    float4 *c = b.compact + (size_t)j * kSurfaceCompactF4 + 2;
    const float alive = c->w;
    *c = make_float4(flux.x * inv_n, flux.y * inv_n, flux.z * inv_n, alive);
}

__global__ __launch_bounds__(256) void surface_prog_fold_kernel(SurfaceProgArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const float4 gp = a.points[4 * (size_t)i];
    if (gp.w == 0.0f) return;                                               // the stencil: not touched at all
    const float4 *s = a.states + 3 * (size_t)i;
    const float4 q0 = s[0]; float4 q1 = s[1], q2 = s[2];
    if (!sp_finite(v3(gp)) || !sp_finite(sp_eye(a, i)) ||
        ((a.what & EVPLP_SURFACE_PHOTONS) && !ss_radius_ok(__float_as_uint(q2.z), q0.w, a.r0sq))) { sp_flag(a.states, i, __float_as_uint(q2.w)); return; }
    const float4 l = a.lights[2 * (size_t)i];
    q1.x += l.x; q1.y += l.y; q1.z += l.z; q2.x += l.w;
    q2.y = __uint_as_float(__float_as_uint(q2.y) + 1u);
    float4 *o = a.states + 3 * (size_t)i;
    o[1] = q1; o[2] = q2;
}

__global__ __launch_bounds__(64) void surface_prog_photon_kernel(SurfaceProgArgs a) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const float4 *pt = a.points + 4 * (size_t)i;
    const float4 gp = pt[0];
    if (gp.w == 0.0f) return;                                               // the stencil: not touched at all
    const V3 eye = sp_eye(a, i);
    const V3 X = v3(gp);
    const SpState raw = sp_load(a.states, i);
    evplp_surface_state st = sp_unpack(raw);
    if (!sp_finite(X) || !sp_finite(eye) || !ss_radius_ok(st.pm_calls, st.radius2, a.r0sq)) { sp_flag(a.states, i, st.flags); return; }
    const float r2 = st.pm_calls == 0u ? a.r0sq : st.radius2;              // the lane's own
    const float xs[3] = { X.x, X.y, X.z };
    int32_t c0[3], c1[3];
    V3 sum = v3(0.f, 0.f, 0.f);
    uint32_t pairs = 0u;
    // (one farther than its reach from the scene's box: M = 0 without touching the table)
    if (pg_range(xs, ss_radius_bound(r2, a.grid.radius), a.grid.lo, a.grid.hi, a.grid.edge, c0, c1)) {
        const float4 gn = pt[1], gd = pt[2], gs = pt[3];
        const V3 sn = v3(gn), sd = v3(gd), sps = v3(gs); const float se = gs.w;
        const V3 w10 = normalize(eye - X);                                  // frag:177
        const uint32_t mode = a.fp.mis_mode;
        const float clampv = a.fp.clamping_value;
        const bool glossy = sps.x != 0.0f || sps.y != 0.0f || sps.z != 0.0f;
        // (surface_state.h: at most two cells wide per axis; the bound keeps the loops finite whatever the inputs)
        for (int k = 0; k < 3; k++) c1[k] = min(c1[k], c0[k] + 2);
        for (int32_t cz = c0[2]; cz <= c1[2]; cz++) for (int32_t cy = c0[1]; cy <= c1[1]; cy++) for (int32_t cx = c0[0]; cx <= c1[0]; cx++) {
            const uint32_t bk = pg_bucket(cx, cy, cz, a.grid.bits);
            const uint32_t jb = a.grid.start[bk], je = a.grid.start[bk + 1u];
            for (uint32_t j = jb; j < je; j++) {
                const float4 *c = a.grid.compact + (size_t)j * kSurfaceCompactF4;
                const float4 c4 = c[4];
                if (__float_as_int(c4.x) != cx || __float_as_int(c4.y) != cy || __float_as_int(c4.z) != cz) continue;       // this cell's photons only
                const float4 q0 = c[0];
                const V3 dv = v3(q0) - X;
                if (dot_exact(dv, dv) > r2) continue;                       // evo_photon_frag's roundings, the lane's radius2
                pairs++;
                const float4 q1 = c[1], q2 = c[2];
                const V3 w12 = v3(q1);
                V3 brdf1 = sp_lambert_eval(w10, w12, sn, sd);               // frag:181
                if (glossy) brdf1 = brdf1 + sp_phong_eval(w10, w12, sn, sps, se);
                if (q2.w == 0.0f) continue;                                 // mixPdfW > 0, frag:191
                V3 col;
                if (mode == 0u) col = brdf1 * v3(q2);
                else {
                    const float cc = fmaxf(dot(sn, w12), 0.0f) * q0.w;      // frag:216,226
                    if (cc <= 0.0f) continue;                               // discard
                    const float g = cc * sp_rcp(q1.w);
                    if (mode == 4u) col = (brdf1 * v3(q2)) * (fmaxf(g - clampv, 0.0f) * sp_rcp(g));
                    else {
                        const V3 brdf2 = v3(c[3]);
                        V3 num = (brdf1 * brdf2) * g;
                        num = v3(fmaxf(num.x - clampv, 0.f), fmaxf(num.y - clampv, 0.f), fmaxf(num.z - clampv, 0.f));
                        const V3 den = brdf2 * g;
                        const V3 pre = v3(q2);
                        // zero denominator contributes 0 (the reference produces NaN here)
                        col = v3(den.x != 0.f ? pre.x * num.x * sp_rcp(den.x) : 0.f, den.y != 0.f ? pre.y * num.y * sp_rcp(den.y) : 0.f,
                                 den.z != 0.f ? pre.z * num.z * sp_rcp(den.z) : 0.f);
                    }
                }
                sum = sum + col;
            }
        }
    }
    const float phi[3] = { sum.x, sum.y, sum.z };
    ss_update(&st, pairs, phi, a.alpha, a.r0sq);
    float4 *o = a.states + 3 * (size_t)i;
    o[0] = make_float4(st.tau[0], st.tau[1], st.tau[2], st.radius2);
    o[1] = make_float4(raw.q1.x, raw.q1.y, raw.q1.z, st.n);
    o[2] = make_float4(raw.q2.x, raw.q2.y, __uint_as_float(st.pm_calls), raw.q2.w);
}

namespace {
EV_DEV void sp_resolve(const float4 *states, size_t i, float4 &l0, float4 &l1) {
    const evplp_surface_state st = sp_unpack(sp_load(states, i));
    evplp_surface_light r;
    ss_resolve(&st, &r);
    l0 = make_float4(r.vpl[0], r.vpl[1], r.vpl[2], r.lit);
    l1 = make_float4(r.pm[0], r.pm[1], r.pm[2], r.photons);
}
}

__global__ __launch_bounds__(256) void surface_prog_resolve_kernel(SurfaceResolveArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    float4 l0, l1;
    sp_resolve(a.states, i, l0, l1);
    a.out[2 * (size_t)i] = l0; a.out[2 * (size_t)i + 1] = l1;
}

__global__ __launch_bounds__(256) void lightmap_prog_resolve_kernel(LightmapProgResolveArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.texels) return;
    float4 vpl = make_float4(0.f, 0.f, 0.f, 0.f), pm = vpl;
    int32_t n = 0;
    for (int32_t s = 0; s < a.s2; s++) {                                    // ascending (j, i): the samples' order in memory
        const size_t at = (size_t)i * (size_t)a.s2 + (size_t)s;
        const float4 q2 = a.states[3 * at + 2];
        if (__float_as_uint(q2.y) + __float_as_uint(q2.z) == 0u || (__float_as_uint(q2.w) & EVPLP_STATE_INVALID)) continue;
        float4 l0, l1;
        sp_resolve(a.states, at, l0, l1);
        vpl.x += l0.x; vpl.y += l0.y; vpl.z += l0.z;
        pm.x += l1.x; pm.y += l1.y; pm.z += l1.z; pm.w += l1.w;
        n++;
    }
    if (n > 0) {
        const float d = (float)n;
        vpl.x = vpl.x / d; vpl.y = vpl.y / d; vpl.z = vpl.z / d; vpl.w = d / (float)a.s2;
        pm.x = pm.x / d; pm.y = pm.y / d; pm.z = pm.z / d; pm.w = pm.w / d;
    }
    float4 *o = reinterpret_cast<float4 *>(a.out + i);
    o[0] = vpl; o[1] = pm;
}

void launch_surface_prog_compact(const SurfaceGridBuild &b, hipStream_t s) {
    if (b.g.slots == 0u) return;
    hipLaunchKernelGGL(surface_prog_compact_kernel, dim3((b.g.slots + 255u) / 256u), dim3(256), 0, s, b);
}
void launch_surface_prog_fold(const SurfaceProgArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(surface_prog_fold_kernel, dim3((uint32_t)(a.n + 255) / 256u), dim3(256), 0, s, a);
}
void launch_surface_prog_photons(const SurfaceProgArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(surface_prog_photon_kernel, dim3((uint32_t)(((int64_t)a.n + 63) / 64)), dim3(64), 0, s, a);
}
void launch_surface_prog_resolve(const SurfaceResolveArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(surface_prog_resolve_kernel, dim3((uint32_t)(((int64_t)a.n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_lightmap_prog_resolve(const LightmapProgResolveArgs &a, hipStream_t s) {
    if (a.texels <= 0) return;
    hipLaunchKernelGGL(lightmap_prog_resolve_kernel, dim3((uint32_t)(((int64_t)a.texels + 255) / 256)), dim3(256), 0, s, a);
}

} // namespace evplp
