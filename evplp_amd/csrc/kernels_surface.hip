// Surface gather (evplp_gather_surface, surface_gather.cpp): the renderer's own two estimates at a caller's surface points.
//   surface_vpl_kernel     <- gather_lvc_kernel's pair (splatColor + vplSplat, rt/lighttracing.cu:348-379, 275-346) in the probe gather's
//                             decomposition: one wave per (64 consecutive points, slice of kSurfaceSlice record slots), lane = point.  The
//                             record is wave-uniform and arrives by scalar loads; an unusable slot is a scalar branch; the shadow ray is
//                             ray_occluded_kernel's instantiation of the per-lane walk, so a pair's visibility is evplp_trace_occluded's answer.
//   surface_cell_kernel    <- per record slot the photon's cell in the world-space grid of photon_grid.h and its bucket key
//   surface_bucket_kernel  <- bucket starts from the sorted keys (the stable radix sort of (key, slot) runs between the two)
//   surface_compact_kernel <- the photon-side terms of the fragment shader (splat_prepare_one of kernels_splat.hip, frag:163-191), in sorted order
//   surface_photon_kernel  <- lane = point: the cells of the point's range in ascending (z, y, x), in each bucket the photons of that very
//                             cell in ascending slot, evo_photon_frag's radius test, the fragment (shaders/photonsplatinstanced.frag:146-240)
//   surface_reduce_kernel  <- the slices' sums in slice order, the division: the first 16 bytes of the record (and the second where no photons are asked for)
// The unit carries its own copy of the pair shading (vpl_shade of kernels_gather.hip, the fragment of kernels_splat.hip), as kernels_probe.hip
// does: those units are built with contraction and hold the frame's registers to their counts; this one is built without (the cosine test's
// sign, the walk's t and the radius test are then the oracle's bits) and nothing of theirs changes.  No float atomics anywhere.
#include "device_common.hpp"
#include "kernels.h"
#include "photon_grid.h"
#include "surface_gather.hpp"

#include <hipcub/hipcub.hpp>

namespace evplp {

#ifndef EVPLP_QUERY_SPEC
#define EVPLP_QUERY_SPEC 1       // kernels_query.hip's setting: the same walk
#endif
#ifndef EVPLP_SURFACE_WAVES
#define EVPLP_SURFACE_WAVES 7    // 72 registers per lane: the kernel takes 71 -- the walk, the receiver's 16 floats, four accumulators -- and spills
                                 // nothing (tests/test_surface_resources.py holds the count); the probe gather's 28 accumulators need 80 and six waves
#endif

namespace {
EV_DEV bool sf_finite(float x) { return fabsf(x) <= 3.4028235e38f; }        // (false for a NaN)
EV_DEV bool sf_finite(V3 x) { return sf_finite(x.x) && sf_finite(x.y) && sf_finite(x.z); }
EV_DEV V3 sf_eye(const SurfaceArgs &a, uint32_t i) {
    if (!a.eyes) return v3(a.fp.camera_pos);
    const float *e = a.eyes + 3 * (size_t)i;
    return v3(e[0], e[1], e[2]);
}

// the record through a wave-uniform base and byte offset, as load_probe_vpl (kernels_probe.hip) spells it out, with the lobe-selection
// probability the MIS modes read
struct SurfVpl { V3 pos, n, flux, fdir, rd, rs; float psel, e; uint32_t flags; };
EV_DEV SurfVpl load_surface_vpl(const evplp_record *base, uint32_t byte_offset) {
    v8i ra; v16i rb;
    asm("s_load_dwordx8 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %3 offset:0x20\n\ts_waitcnt lgkmcnt(0)" : "=&s"(ra), "=&s"(rb) : "s"(base), "s"(byte_offset));
    SurfVpl v;
    v.pos = v3(f_of(ra[0]), f_of(ra[1]), f_of(ra[2])); v.flags = (uint32_t)ra[3]; v.n = v3(f_of(ra[4]), f_of(ra[5]), f_of(ra[6])); v.psel = f_of(ra[7]);
    v.flux = v3(f_of(rb[0]), f_of(rb[1]), f_of(rb[2])); v.fdir = v3(f_of(rb[4]), f_of(rb[5]), f_of(rb[6]));
    v.rd = v3(f_of(rb[8]), f_of(rb[9]), f_of(rb[10])); v.rs = v3(f_of(rb[12]), f_of(rb[13]), f_of(rb[14])); v.e = f_of(rb[15]);
    return v;
}
struct SurfPoint { V3 p1, n1, rd, rs; float e; V3 wi10; };
// PhongEvalF (rtmaterial.cuh:112-118) with the power on the hardware transcendentals, as phong_eval_f_hw of kernels_gather.hip
EV_DEV float sf_phong_f(V3 out, V3 in, V3 n, float e) {
    const V3 r = reflect(-in, n);
    const float d = fmaxf(dot(out, r), 0.0f);
    if (d <= 0.000001f) return 0.0f;
    return (e + 2.0f) * __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(d)) * EV_INV_PI * 0.5f;
}
// vplSplat after the visibility test (rt/lighttracing.cu:296-345): vpl_shade of kernels_gather.hip, operation for operation
EV_DEV V3 surface_vpl_shade(const evplp_frame_params &fp, float pdf_mc2, const SurfPoint &px, const SurfVpl &v, V3 v12, float c1c2, bool px_glossy) {
    const float dist2 = dot(v12, v12);
    const V3 wi12 = v12 * __builtin_amdgcn_rsqf(dist2);
    float ph2 = 0.0f;
    if (v.rs.x != 0.0f || v.rs.y != 0.0f || v.rs.z != 0.0f) {              // wave-uniform (the VPL is)
        if (v.e == 0.0f) { const V3 r = reflect(-v.fdir, v.n); ph2 = fmaxf(dot(-wi12, r), 0.0f) <= 0.000001f ? 0.0f : (v.e + 2.0f) * 1.0f * EV_INV_PI * 0.5f; }
        else ph2 = sf_phong_f(-wi12, v.fdir, v.n, v.e);
    }
    float ph1 = 0.0f;
    if (px_glossy) ph1 = sf_phong_f(px.wi10, wi12, px.n1, px.e);             // wave-uniform: some point of the wave has a lobe (rho_s = 0 makes the term exactly 0)
    const V3 brdf2 = v.rd * EV_INV_PI + v.rs * ph2;
    const V3 brdf1 = px.rd * EV_INV_PI + px.rs * ph1;
    const float g21 = c1c2 * __builtin_amdgcn_rcpf(dist2 * dist2);
    const uint32_t mode = fp.mis_mode;
    if (mode == 0u) return v.flux * brdf1 * brdf2 * g21;
    if (mode <= 3u) {
        float pdf_de = g21 * EV_INV_PI * v.psel;
        if (!(v.rs.x <= 0.000001f))
            pdf_de += ph2 * ((v.e + 1.0f) * __builtin_amdgcn_rcpf(v.e + 2.0f)) * fmaxf(dot(px.n1, wi12), 0.0f) * __builtin_amdgcn_rcpf(dist2) * (1.0f - v.psel);
        float w;
        if (mode == 1u) w = fp.pdf_mc * __builtin_amdgcn_rcpf(fp.pdf_mc + pdf_de);
        else if (mode == 2u) w = fp.pdf_mc > pdf_de ? 1.0f : 0.0f;
        else { const float a2 = pdf_mc2, b2 = pdf_de * pdf_de; w = a2 * __builtin_amdgcn_rcpf(a2 + b2); }
        return (v.flux * w) * brdf1 * brdf2 * g21;
    }
    if (mode == 4u) return (v.flux * fminf(g21, fp.clamping_value)) * brdf1 * brdf2;
    V3 x = (brdf1 * g21) * brdf2;
    x = v3(fminf(x.x, fp.clamping_value), fminf(x.y, fp.clamping_value), fminf(x.z, fp.clamping_value));
    return v.flux * x;
}

// the fragment shader's helpers (photonsplatinstanced.frag:42-98), as kernels_splat.hip has them
EV_DEV float sf_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
EV_DEV V3 sf_normalize_hw(V3 v) { return v * __builtin_amdgcn_rsqf(dot(v, v)); }
EV_DEV float sf_pow(float d, float e) { return e == 0.0f ? 1.0f : __builtin_amdgcn_exp2f(e * __builtin_amdgcn_logf(d)); }
EV_DEV V3 sf_lambert_eval(V3 w10, V3 w12, V3 n, V3 rd) {
    if (dot(w10, n) <= 0.0f || dot(w12, n) <= 0.0f) return v3(0.f, 0.f, 0.f);
    return rd * EV_INV_PI;
}
EV_DEV V3 sf_phong_eval(V3 outv, V3 inv_, V3 n, V3 rs, float e) {
    const V3 r = reflect(-inv_, n);
    const float d = dot(outv, r);
    if (d <= 0.00001f) return v3(0.f, 0.f, 0.f);
    return rs * (e + 2.0f) * sf_pow(d, e) * EV_INV_PI * 0.5f;
}
EV_DEV float sf_lambert_pdf_w(V3 n1, V3 v12) { return fmaxf(dot(n1, sf_normalize_hw(v12)), 0.f) * EV_INV_PI; }
EV_DEV float sf_phong_pdf_w(V3 n1, V3 wi12, V3 inv_, V3 rs, float e) {
    const V3 r = reflect(-inv_, n1);
    const float d = fmaxf(dot(wi12, r), 0.f);
    if (d <= 0.00001f || rs.x <= 0.00001f) return 0.0f;
    return (e + 1.0f) * 0.5f * EV_INV_PI * sf_pow(d, e);
}
struct SurfRec { V3 pos, n, flux, fdir, rd, rs; float psel, e; };
EV_DEV SurfRec load_surface_rec(const evplp_record *r) {
    const float4 *q = reinterpret_cast<const float4 *>(r);
    const float4 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4], f = q[5];
    SurfRec v; v.pos = v3(a); v.n = v3(b); v.psel = b.w; v.flux = v3(c); v.fdir = v3(d); v.rd = v3(e); v.rs = v3(f); v.e = f.w;
    return v;
}
}

__global__ __launch_bounds__(64, EVPLP_SURFACE_WAVES) void surface_vpl_kernel(SurfaceArgs a) {
    extern __shared__ int32_t lds_stack[];   // [surface_stack_bytes / 256][64 lanes]
    const int lane = threadIdx.x;
    const uint32_t slice = blockIdx.x;
    const uint32_t i = blockIdx.y * 64u + lane;
    if (i >= (uint32_t)a.n) return;
    const float4 *pt = a.points + 4 * (size_t)i;
    const float4 gp = pt[0];
    const V3 eye = sf_eye(a, i);
    // (the reduce decides both from the same floats and reads no partial sum of such a point)
    if (gp.w == 0.0f || !sf_finite(v3(gp)) || !sf_finite(eye)) return;      // stencil (:354); never walked
    const float4 gn = pt[1], gd = pt[2], gs = pt[3];
    SurfPoint px;
    px.p1 = v3(gp); px.n1 = v3(gn); px.rd = v3(gd); px.rs = v3(gs); px.e = gs.w;
    px.wi10 = normalize(eye - px.p1);                                       // :363
    const bool px_glossy = ballot64(px.rs.x != 0.0f || px.rs.y != 0.0f || px.rs.z != 0.0f) != 0ull;
    const uint32_t first = slice * kSurfaceSlice;
    const uint32_t end = a.slots - first < kSurfaceSlice ? a.slots : first + kSurfaceSlice;     // (first < slots: the launch has ceil(slots / slice) slices)
    float sr = 0.f, sg = 0.f, sb = 0.f, lit = 0.f;
    const evplp_record *slice_records = pinned(a.records + first);
    for (uint32_t k = first; k < end; k++) {
        const SurfVpl v = load_surface_vpl(slice_records, (k - first) * (uint32_t)sizeof(evplp_record));       // wave-uniform
        if ((v.flags & (uint32_t)EVPLP_USABLE_VPL) == 0u) continue;              // a scalar branch
        const V3 v12 = v.pos - px.p1;
        const float c1 = fmaxf(dot_exact(px.n1, v12), 0.0f);
        const float c2 = fmaxf(-dot_exact(v.n, v12), 0.0f);
        const float c1c2 = c1 * c2;
        if (c1c2 <= 0.0f) continue;
        if (occluded_lane4<64, EVPLP_QUERY_SPEC, true>(a.sc, v.pos, -v12, 0.0001f, 1.0f - 0.0001f, lds_stack + lane)) continue;
        const V3 c = surface_vpl_shade(a.fp, a.pdf_mc2, px, v, v12, c1c2, px_glossy);
        sr += c.x; sg += c.y; sb += c.z; lit += 1.0f;
    }
    float *p = a.partial + (size_t)slice * 4 * kSurfaceChunk + i;           // [slice][4][point]: a wave's 64 floats are one 256-byte line
    const size_t s = kSurfaceChunk;
    p[0 * s] = sr; p[1 * s] = sg; p[2 * s] = sb; p[3 * s] = lit;
}

// ------------------------------------------------------------------------------------------------------------------ the grid
__global__ __launch_bounds__(256) void surface_cell_kernel(SurfaceGridBuild b) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= b.g.slots) return;
    const float4 a = *reinterpret_cast<const float4 *>(b.records + i);
    // (slot 0 has no predecessor on its path: never a photon, as in evplp_splat_photons)
    const bool usable = i != 0u && (__float_as_uint(a.w) & (uint32_t)EVPLP_USABLE_PHOTON) != 0u;
    uint32_t key = 1u << b.g.bits;                                          // behind every bucket
    if (usable) key = pg_bucket(pg_cell1(a.x, b.g.lo[0], b.g.edge), pg_cell1(a.y, b.g.lo[1], b.g.edge), pg_cell1(a.z, b.g.lo[2], b.g.edge), b.g.bits);
    b.keys[i] = key; b.vals[i] = i;
}
// start[q] = the first sorted position whose key is >= q, for q in [0, 2^bits + 1]: one thread per entry, a bisection of the sorted keys --
// log2(slots) steps whatever the photons' distribution (one thread per sorted position, writing the keys up to its own, runs as long as
// the widest gap: a whole table when every photon shares a cell)
__global__ __launch_bounds__(256) void surface_bucket_kernel(SurfaceGridBuild b) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q > (1u << b.g.bits) + 1u) return;
    uint32_t lo = 0u, hi = b.g.slots;                                       // the answer lies in [lo, hi]
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (b.keys_sorted[mid] < q) lo = mid + 1u; else hi = mid; }
    b.start[q] = lo;
}
// compact photon: [0] pos.xyz, cpn   [1] w12.xyz, d2   [2] wflux.xyz, alive   [3] brdf2.xyz (misMode 5 reads it)   [4] cell, slot
__global__ __launch_bounds__(256) void surface_compact_kernel(SurfaceGridBuild b) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= b.g.slots) return;
    if (b.keys_sorted[j] >> b.g.bits) return;                               // an unusable slot: nothing reads its record
    const uint32_t i = b.vals_sorted[j];
    const SurfRec ph = load_surface_rec(b.records + i), prev = load_surface_rec(b.records + i - 1u);     // frag:163
    const float r = b.fp.photon_radius;
    const V3 v12 = prev.pos - ph.pos;                                       // frag:170
    const float d2 = dot(v12, v12);
    const V3 w12 = sf_normalize_hw(v12);
    float mix_w = sf_lambert_pdf_w(prev.n, -w12) * prev.psel;               // frag:184-187
    mix_w += sf_phong_pdf_w(prev.n, -w12, prev.fdir, prev.rs, prev.e) * (1.0f - prev.psel);
    const float mix_a = mix_w * fmaxf(dot(ph.n, w12), 0.0f) * sf_rcp(d2);   // frag:189
    const bool alive = mix_w > 0.0f;                                        // frag:191
    const float k = EV_INV_PI * sf_rcp(r * r);                              // InvPi * uInvPhotonRadius2
    const float inv_n = sf_rcp((float)b.fp.num_light_paths);                // uInvNumLightPaths
    float wgt = 1.0f;
    const uint32_t mode = b.fp.mis_mode;
    if (mode == 1u) wgt = mix_a * sf_rcp(mix_a + b.fp.pdf_mc);
    else if (mode == 2u) wgt = mix_a > b.fp.pdf_mc ? 1.0f : 0.0f;
    else if (mode == 3u) { const float a2 = mix_a * mix_a, b2 = b.fp.pdf_mc * b.fp.pdf_mc; wgt = a2 * sf_rcp(a2 + b2); }
    const V3 wflux = ph.flux * (k * inv_n * wgt);
    const float cpn = fmaxf(-dot(prev.n, w12), 0.0f);
    const V3 brdf2 = sf_lambert_eval(-w12, prev.fdir, prev.n, prev.rd) + sf_phong_eval(-w12, prev.fdir, prev.n, prev.rs, prev.e);  // frag:182
    float4 *c = b.compact + (size_t)j * kSurfaceCompactF4;
    c[0] = make_float4(ph.pos.x, ph.pos.y, ph.pos.z, cpn);
    c[1] = make_float4(w12.x, w12.y, w12.z, d2);
    c[2] = make_float4(wflux.x, wflux.y, wflux.z, alive ? 1.0f : 0.0f);
    c[3] = make_float4(brdf2.x, brdf2.y, brdf2.z, 0.f);
    c[4] = make_float4(__int_as_float(pg_cell1(ph.pos.x, b.g.lo[0], b.g.edge)), __int_as_float(pg_cell1(ph.pos.y, b.g.lo[1], b.g.edge)),
                       __int_as_float(pg_cell1(ph.pos.z, b.g.lo[2], b.g.edge)), __uint_as_float(i));
}

// ------------------------------------------------------------------------------------------------------------------ the query
// One wave per workgroup: a launch of one chunk is 256 waves, one per CU, where four-wave workgroups left three CUs in four idle (measured:
// 83 us per chunk of 16 384 points with 256 threads a workgroup).  The kernel answers its half for EVERY point -- zeros for a stencilled one,
// zeros and -1 for one that is not finite -- as the second 16 bytes of the record; the reduce leaves them alone.
__global__ __launch_bounds__(64) void surface_photon_kernel(SurfaceArgs a) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const float4 *pt = a.points + 4 * (size_t)i;
    const float4 gp = pt[0];
    const V3 eye = sf_eye(a, i);
    const V3 X = v3(gp);
    const bool finite = sf_finite(X) && sf_finite(eye);
    float4 res = make_float4(0.f, 0.f, 0.f, gp.w != 0.0f && !finite ? -1.0f : 0.0f);
    const float xs[3] = { X.x, X.y, X.z };
    int32_t c0[3], c1[3];
    // (a stencilled point, one that is not finite, one farther than the reach from the scene's box: answered without touching the table)
    if (gp.w != 0.0f && finite && pg_range(xs, a.grid.radius, a.grid.lo, a.grid.hi, a.grid.edge, c0, c1)) {
        const float4 gn = pt[1], gd = pt[2], gs = pt[3];
        const V3 sn = v3(gn), sd = v3(gd), sps = v3(gs); const float se = gs.w;
        const V3 w10 = normalize(eye - X);                                  // frag:177
        const float r2 = a.fp.photon_radius * a.fp.photon_radius;           // frag:152
        const uint32_t mode = a.fp.mis_mode;
        const float clampv = a.fp.clamping_value;
        const bool glossy = sps.x != 0.0f || sps.y != 0.0f || sps.z != 0.0f;
        V3 sum = v3(0.f, 0.f, 0.f);
        uint32_t pairs = 0u;
        // (photon_grid.h proves a walked point's range at most two cells wide per axis; the bound keeps the loops finite whatever the inputs)
        for (int k = 0; k < 3; k++) c1[k] = min(c1[k], c0[k] + 2);
        for (int32_t cz = c0[2]; cz <= c1[2]; cz++) for (int32_t cy = c0[1]; cy <= c1[1]; cy++) for (int32_t cx = c0[0]; cx <= c1[0]; cx++) {
            const uint32_t bk = pg_bucket(cx, cy, cz, a.grid.bits);
            const uint32_t jb = a.grid.start[bk], je = a.grid.start[bk + 1u];
            for (uint32_t j = jb; j < je; j++) {
                const float4 *c = a.grid.compact + (size_t)j * kSurfaceCompactF4;
                const float4 c4 = c[4];
                // the bucket's photons of THIS cell only: a collision, or two cells of the range in one bucket, costs time and nothing else
                if (__float_as_int(c4.x) != cx || __float_as_int(c4.y) != cy || __float_as_int(c4.z) != cz) continue;
                const float4 q0 = c[0];
                const V3 dv = v3(q0) - X;
                if (dot_exact(dv, dv) > r2) continue;                       // frag:153-154, evo_photon_frag's roundings
                pairs++;
                const float4 q1 = c[1], q2 = c[2];
                const V3 w12 = v3(q1);
                V3 brdf1 = sf_lambert_eval(w10, w12, sn, sd);               // frag:181
                if (glossy) brdf1 = brdf1 + sf_phong_eval(w10, w12, sn, sps, se);
                if (q2.w == 0.0f) continue;                                 // mixPdfW > 0, frag:191
                V3 col;
                if (mode <= 3u) col = brdf1 * v3(q2);
                else {
                    const float cc = fmaxf(dot(sn, w12), 0.0f) * q0.w;      // frag:216,226
                    if (cc <= 0.0f) continue;                               // discard
                    const float g = cc * sf_rcp(q1.w);
                    if (mode == 4u) col = (brdf1 * v3(q2)) * (fmaxf(g - clampv, 0.0f) * sf_rcp(g));
                    else {
                        const V3 brdf2 = v3(c[3]);
                        V3 num = (brdf1 * brdf2) * g;
                        num = v3(fmaxf(num.x - clampv, 0.f), fmaxf(num.y - clampv, 0.f), fmaxf(num.z - clampv, 0.f));
                        const V3 den = brdf2 * g;
                        const V3 pre = v3(q2);
                        // zero denominator contributes 0 (the reference produces NaN here)
                        col = v3(den.x != 0.f ? pre.x * num.x * sf_rcp(den.x) : 0.f, den.y != 0.f ? pre.y * num.y * sf_rcp(den.y) : 0.f,
                                 den.z != 0.f ? pre.z * num.z * sf_rcp(den.z) : 0.f);
                    }
                }
                sum = sum + col;
            }
        }
        res = make_float4(sum.x, sum.y, sum.z, (float)pairs);
    }
    reinterpret_cast<float4 *>(a.out + i)[1] = res;
}

__global__ __launch_bounds__(256) void surface_reduce_kernel(SurfaceArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const float4 gp = a.points[4 * (size_t)i];
    const bool finite = sf_finite(v3(gp)) && sf_finite(sf_eye(a, i));
    float4 vpl = make_float4(0.f, 0.f, 0.f, 0.f), pm = vpl;
    if (!finite) { if (gp.w != 0.0f) { vpl.w = -1.0f; pm.w = -1.0f; } }     // (a stencilled point answers eight zeros whatever else it holds)
    else if (gp.w != 0.0f) {
        if (a.what & EVPLP_SURFACE_VPL) {
            for (uint32_t sl = 0; sl < a.slices; sl++) {                    // slice order
                const float *p = a.partial + (size_t)sl * 4 * kSurfaceChunk + i;
                vpl.x += p[0]; vpl.y += p[(size_t)kSurfaceChunk]; vpl.z += p[2 * (size_t)kSurfaceChunk]; vpl.w += p[3 * (size_t)kSurfaceChunk];
            }
            vpl.x = vpl.x / a.paths; vpl.y = vpl.y / a.paths; vpl.z = vpl.z / a.paths;
        }
    }
    float4 *o = reinterpret_cast<float4 *>(a.out + i);
    o[0] = vpl;
    if (!(a.what & EVPLP_SURFACE_PHOTONS)) o[1] = make_float4(0.f, 0.f, 0.f, pm.w);      // (else surface_photon_kernel wrote it)
}

size_t surface_stack_bytes(const SceneDev &sc) { return lane_stack_bytes4(sc); }
size_t surface_sort_temp_bytes(uint32_t slots, uint32_t bits) {
    size_t need = 0;
    uint32_t *none = nullptr;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, need, none, none, none, none, slots, 0, (int)bits + 1, (hipStream_t) nullptr) != hipSuccess) return 0;
    return need;
}
hipError_t launch_surface_grid(const SurfaceGridBuild &b, hipStream_t s) {
    if (b.g.slots == 0u) return hipSuccess;
    const dim3 grid((b.g.slots + 255u) / 256u), block(256);
    hipLaunchKernelGGL(surface_cell_kernel, grid, block, 0, s, b);
    size_t bytes = b.temp_bytes;
    // (a radix sort is stable: equal keys stay in slot order)
    const hipError_t e = hipcub::DeviceRadixSort::SortPairs(b.temp, bytes, b.keys, b.keys_sorted, b.vals, b.vals_sorted, b.g.slots, 0, (int)b.g.bits + 1, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(surface_bucket_kernel, dim3(((1u << b.g.bits) + 2u + 255u) / 256u), block, 0, s, b);
    hipLaunchKernelGGL(surface_compact_kernel, grid, block, 0, s, b);
    return hipSuccess;
}
void launch_surface_vpl(const SurfaceArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.slices == 0) return;
    hipLaunchKernelGGL(surface_vpl_kernel, dim3(a.slices, (uint32_t)(a.n + 63) / 64u), dim3(64), surface_stack_bytes(a.sc), s, a);
}
void launch_surface_photons(const SurfaceArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(surface_photon_kernel, dim3((uint32_t)(((int64_t)a.n + 63) / 64)), dim3(64), 0, s, a);
}
void launch_surface_reduce(const SurfaceArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(surface_reduce_kernel, dim3((uint32_t)(a.n + 255) / 256u), dim3(256), 0, s, a);
}

} // namespace evplp
