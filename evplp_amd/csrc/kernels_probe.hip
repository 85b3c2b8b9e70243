// Probe gather (evplp_gather_probes, probe_gather.cpp): the VPL records' light at free-standing points, as order-2 spherical harmonics.
//   probe_gather_kernel  <- gather_lvc_kernel's pair arithmetic with the receiver taken away: one wave per (64 consecutive probes, slice of
//                           kProbeSlice record slots), lane = probe.  The record is wave-uniform and arrives by scalar loads; an unusable
//                           slot is a scalar branch.  The shadow ray is ray_occluded_kernel's instantiation of the per-lane walk
//                           (occluded_lane4<64, EVPLP_QUERY_SPEC, true>), so a pair's visibility is what evplp_trace_occluded answers.
//   probe_reduce_kernel  <- the slices' partial sums added in slice order, the division by the path count, one 112-byte record out.
// A slice is summed in slot order in fp32 and the slices in index order: a probe's bytes are a function of its position, the records and
// the tree, whatever the batch (include/evplp.h).  The unit is built without floating-point contraction, as kernels_query.hip is: the
// cosine test's sign and the walk's t are then the oracle's bits, and the sums have one rounding per written operation.
#include "device_common.hpp"
#include "kernels.h"
#include "probe_gather.hpp"

namespace evplp {

#ifndef EVPLP_QUERY_SPEC
#define EVPLP_QUERY_SPEC 1       // kernels_query.hip's setting: the same walk
#endif
#ifndef EVPLP_PROBE_WAVES
#define EVPLP_PROBE_WAVES 6      // 80 registers per lane: the kernel takes exactly that -- the walk's 54 less what only a ray batch needs, the probe, 28
                                 // accumulators -- and spills nothing; at 5 it takes 81 (tests/test_probe_resources.py holds the count)
#endif

namespace {
EV_DEV bool probe_finite(float x) { return fabsf(x) <= 3.4028235e38f; }      // (false for a NaN)
EV_DEV bool probe_valid(V3 x) { return probe_finite(x.x) && probe_finite(x.y) && probe_finite(x.z); }
EV_DEV bool probe_walked(float dist2) { return dist2 >= 1.17549435e-38f && dist2 <= 3.4028235e38f; }      // 2^-126 <= dist2 <= FLT_MAX (false for a NaN)

// the VPL side of a record through a wave-uniform base and byte offset: s_load_dwordx8 (position, flags, normal) and s_load_dwordx16
// (the shading fields) issued together and waited for once, spelled out as device_common.hpp's sload8 / sload16 are -- left to the
// compiler the fetch came out as six vector loads per lane
struct ProbeVpl { V3 pos, n, flux, fdir, rd, rs; float e; uint32_t flags; };
EV_DEV ProbeVpl load_probe_vpl(const evplp_record *base, uint32_t byte_offset) {
    v8i ra; v16i rb;
    asm("s_load_dwordx8 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %3 offset:0x20\n\ts_waitcnt lgkmcnt(0)" : "=&s"(ra), "=&s"(rb) : "s"(base), "s"(byte_offset));
    ProbeVpl v;
    v.pos = v3(f_of(ra[0]), f_of(ra[1]), f_of(ra[2])); v.flags = (uint32_t)ra[3]; v.n = v3(f_of(ra[4]), f_of(ra[5]), f_of(ra[6]));
    v.flux = v3(f_of(rb[0]), f_of(rb[1]), f_of(rb[2])); v.fdir = v3(f_of(rb[4]), f_of(rb[5]), f_of(rb[6]));
    v.rd = v3(f_of(rb[8]), f_of(rb[9]), f_of(rb[10])); v.rs = v3(f_of(rb[12]), f_of(rb[13]), f_of(rb[14])); v.e = f_of(rb[15]);
    return v;
}
// PhongEvalF (rtmaterial.cuh:112-118) of the VPL's lobe towards -w as vpl_shade (kernels_gather.hip) takes it: nothing for rho_s = 0 (the
// product would be exactly 0), powf(d, 0) = 1 without the transcendentals, else d^e = exp2(e log2 d) on the hardware
EV_DEV float probe_phong(const ProbeVpl &v, V3 w) {
    if (!(v.rs.x != 0.0f || v.rs.y != 0.0f || v.rs.z != 0.0f)) return 0.0f;        // wave-uniform (the VPL is)
    const V3 r = reflect(-v.fdir, v.n);
    const float d = fmaxf(dot(-w, r), 0.0f);
    if (d <= 0.000001f) return 0.0f;
    if (v.e == 0.0f) return (v.e + 2.0f) * 1.0f * EV_INV_PI * 0.5f;
    return (v.e + 2.0f) * __builtin_amdgcn_exp2f(v.e * __builtin_amdgcn_logf(d)) * EV_INV_PI * 0.5f;
}
}

__global__ __launch_bounds__(64, EVPLP_PROBE_WAVES) void probe_gather_kernel(ProbeArgs a) {
    extern __shared__ int32_t lds_stack[];   // [probe_stack_bytes / 256][64 lanes]
    const int lane = threadIdx.x;
    const uint32_t slice = blockIdx.x;
    const uint32_t i = blockIdx.y * 64u + lane;
    if (i >= (uint32_t)a.n) return;
    const float *xp = a.positions + 3 * (size_t)i;
    const V3 x = v3(xp[0], xp[1], xp[2]);
    if (!probe_valid(x)) return;             // (the reduce decides the same from the same floats and reads no partial sum of this probe)
    const uint32_t first = slice * kProbeSlice;
    const uint32_t end = a.slots - first < kProbeSlice ? a.slots : first + kProbeSlice;     // (first < slots: the launch has ceil(slots / slice) slices)
    float c0r = 0.f, c0g = 0.f, c0b = 0.f, c1r = 0.f, c1g = 0.f, c1b = 0.f, c2r = 0.f, c2g = 0.f, c2b = 0.f;
    float c3r = 0.f, c3g = 0.f, c3b = 0.f, c4r = 0.f, c4g = 0.f, c4b = 0.f, c5r = 0.f, c5g = 0.f, c5b = 0.f;
    float c6r = 0.f, c6g = 0.f, c6b = 0.f, c7r = 0.f, c7g = 0.f, c7b = 0.f, c8r = 0.f, c8g = 0.f, c8b = 0.f;
    float lit = 0.f;
    const evplp_record *slice_records = pinned(a.records + first);
    for (uint32_t k = first; k < end; k++) {
        const ProbeVpl v = load_probe_vpl(slice_records, (k - first) * (uint32_t)sizeof(evplp_record));       // wave-uniform
        if ((v.flags & (uint32_t)EVPLP_USABLE_VPL) == 0u) continue;              // a scalar branch
        const V3 v12 = v.pos - x;
        const float c2 = fmaxf(-dot_exact(v.n, v12), 0.0f);
        if (c2 <= 0.0f) continue;
        // a pair whose dist2 is not a normal finite number casts no ray, adds no term and is not counted (include/evplp.h): every ray walked
        // is then one evplp_trace_occluded accepts, and rsq, w, cos2 and the rcp below stay finite.  dist2 is formed again after the walk
        // (the same bits: the unit is uncontracted), so nothing more is live across it
        if (!probe_walked(dot(v12, v12))) continue;
        if (occluded_lane4<64, EVPLP_QUERY_SPEC, true>(a.sc, v.pos, -v12, 0.0001f, 1.0f - 0.0001f, lds_stack + lane)) continue;
        const float dist2 = dot(v12, v12);
        const float inv_dist = __builtin_amdgcn_rsqf(dist2);
        const V3 w = v12 * inv_dist;
        const float cos2 = c2 * inv_dist;
        const float ph2 = probe_phong(v, w);
        const V3 brdf2 = v.rd * EV_INV_PI + v.rs * ph2;
        const float g = cos2 * __builtin_amdgcn_rcpf(fmaxf(dist2, a.min_dist2));
        const V3 E = (v.flux * brdf2) * g;
        const float y0 = 0.28209479f, y1 = 0.48860251f * w.y, y2 = 0.48860251f * w.z, y3 = 0.48860251f * w.x;
        const float y4 = 1.09254843f * (w.x * w.y), y5 = 1.09254843f * (w.y * w.z), y6 = 0.31539157f * (3.0f * (w.z * w.z) - 1.0f);
        const float y7 = 1.09254843f * (w.x * w.z), y8 = 0.54627422f * (w.x * w.x - w.y * w.y);
        c0r += E.x * y0; c0g += E.y * y0; c0b += E.z * y0;
        c1r += E.x * y1; c1g += E.y * y1; c1b += E.z * y1;
        c2r += E.x * y2; c2g += E.y * y2; c2b += E.z * y2;
        c3r += E.x * y3; c3g += E.y * y3; c3b += E.z * y3;
        c4r += E.x * y4; c4g += E.y * y4; c4b += E.z * y4;
        c5r += E.x * y5; c5g += E.y * y5; c5b += E.z * y5;
        c6r += E.x * y6; c6g += E.y * y6; c6b += E.z * y6;
        c7r += E.x * y7; c7g += E.y * y7; c7b += E.z * y7;
        c8r += E.x * y8; c8g += E.y * y8; c8b += E.z * y8;
        lit += 1.0f;
    }
    float *p = a.partial + (size_t)slice * kProbeFloats * kProbeChunk + i;       // [slice][float][probe]: a wave's 64 floats are one 256-byte line
    const size_t s = kProbeChunk;
    p[0 * s] = c0r; p[1 * s] = c0g; p[2 * s] = c0b; p[3 * s] = c1r; p[4 * s] = c1g; p[5 * s] = c1b; p[6 * s] = c2r; p[7 * s] = c2g; p[8 * s] = c2b;
    p[9 * s] = c3r; p[10 * s] = c3g; p[11 * s] = c3b; p[12 * s] = c4r; p[13 * s] = c4g; p[14 * s] = c4b; p[15 * s] = c5r; p[16 * s] = c5g; p[17 * s] = c5b;
    p[18 * s] = c6r; p[19 * s] = c6g; p[20 * s] = c6b; p[21 * s] = c7r; p[22 * s] = c7g; p[23 * s] = c7b; p[24 * s] = c8r; p[25 * s] = c8g; p[26 * s] = c8b;
    p[27 * s] = lit;
}

__global__ __launch_bounds__(256) void probe_reduce_kernel(ProbeArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const float *xp = a.positions + 3 * (size_t)i;
    const bool valid = probe_valid(v3(xp[0], xp[1], xp[2]));
    float sum[kProbeFloats];
#pragma unroll
    for (int f = 0; f < kProbeFloats; f++) sum[f] = 0.0f;
    if (valid) {
        for (uint32_t sl = 0; sl < a.slices; sl++) {                             // slice order
            const float *p = a.partial + (size_t)sl * kProbeFloats * kProbeChunk + i;
#pragma unroll
            for (int f = 0; f < kProbeFloats; f++) sum[f] += p[(size_t)f * kProbeChunk];
        }
#pragma unroll
        for (int f = 0; f < kProbeFloats - 1; f++) sum[f] = sum[f] / a.paths;
    } else sum[kProbeFloats - 1] = -1.0f;
    float4 *o = reinterpret_cast<float4 *>(a.out + i);
#pragma unroll
    for (int q = 0; q < kProbeFloats / 4; q++) o[q] = make_float4(sum[4 * q], sum[4 * q + 1], sum[4 * q + 2], sum[4 * q + 3]);
}

size_t probe_stack_bytes(const SceneDev &sc) { return lane_stack_bytes4(sc); }
void launch_probe_gather(const ProbeArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.slices == 0) return;
    hipLaunchKernelGGL(probe_gather_kernel, dim3(a.slices, (uint32_t)(a.n + 63) / 64u), dim3(64), probe_stack_bytes(a.sc), s, a);
}
void launch_probe_reduce(const ProbeArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(probe_reduce_kernel, dim3((uint32_t)(a.n + 255) / 256u), dim3(256), 0, s, a);
}

} // namespace evplp
