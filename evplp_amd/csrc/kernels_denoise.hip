// Edge-aware denoiser of a written frame (evplp_denoise, include/evplp.h): the spatial part of SVGF (Schied et al. 2017), an a-trous
// wavelet filter (Dammertz et al. 2010) guided by the G-buffer and by the per-pixel variance of the noise tracker.
//   denoise_prepare_kernel  one thread per pixel of a context's planes: demodulates the composite by the albedo and packs the pass inputs
//   denoise_level_kernel    one launch per a-trous pass over the whole frame, 5 x 5 taps at step h, ping-ponging two planes
//   denoise_finish_kernel   remodulates the filtered pixels and copies the others from the composite
// The packed pixel (DenoisePixel, kernels.h) carries everything the passes read, so that the strips of a group can be exchanged and assembled
// as plain floats.  Every sum is taken in a fixed order, without atomics: a call is bit-reproducible.  The file is compiled without
// floating-point contraction, so that the restatement in tests/denoise_hostile.py can follow the operation order.
// No LDS staging: a pass reads 48 B per tap (u, position, normal) of a frame of 80 B per pixel (74 MB at 1280 x 720), which stays in the
// Infinity Cache across the passes, and neighbouring lanes read neighbouring pixels; the passes are measured (tools/denoise_gain.py).
#include "kernels.h"

namespace evplp {

namespace {
constexpr float kLumR = 0.2126f, kLumG = 0.7152f, kLumB = 0.0722f;
__device__ inline float luminance(float r, float g, float b) { return (kLumR * r + kLumG * g) + kLumB * b; }
__device__ inline bool is_finite(float x) { return fabsf(x) <= 3.4028235e38f; }       // false for Inf and for NaN
}

// rgb: the composite (scale, scale, light_scale, mask_emitter, no gamma), var: the noise tracker's variance at `scale`, both 3 floats per
// plane pixel; the guides and the light plane of the same pixels.  Filtered: an image row, a surface (position.w != 0), no emitter, and a
// finite (u, s).
__global__ __launch_bounds__(256) void denoise_prepare_kernel(StripDev st, const float *rgb, const float *var, const float4 *pos, const float4 *nrm,
                                                              const float4 *dif, const float4 *phg, const float4 *light, float4 *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)st.W * st.local_rows;
    if (i >= n) return;
    const int y = st.global_row((int)(i / (size_t)st.W));
    const float4 p = pos[i], nn = nrm[i], d = dif[i], ph = phg[i], li = light[i];
    bool filtered = y < st.H && p.w != 0.0f && li.x == 0.0f && li.y == 0.0f && li.z == 0.0f;
    const float c[3] = { rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2] };
    const float a[3] = { fmaxf(d.x + ph.x, 1e-3f), fmaxf(d.y + ph.y, 1e-3f), fmaxf(d.z + ph.z, 1e-3f) };
    float4 u = make_float4(c[0], c[1], c[2], 0.0f);
    if (filtered) {
        float4 v;
        v.x = c[0] / a[0]; v.y = c[1] / a[1]; v.z = c[2] / a[2];
        v.w = ((kLumR * kLumR) * var[3 * i] / (a[0] * a[0]) + (kLumG * kLumG) * var[3 * i + 1] / (a[1] * a[1])) + (kLumB * kLumB) * var[3 * i + 2] / (a[2] * a[2]);
        // a demodulated colour or an s that is not finite (an overflowed sample, c / a beyond fp32, a variance beyond fp32): not filtered.
        // As a tap it would be weight 0 times Inf, a NaN in every pixel that reaches it, at every pass; position.w = 0 keeps it out of
        // the passes, of the temporal accumulation and of the history alike.
        filtered = is_finite(v.x) && is_finite(v.y) && is_finite(v.z) && is_finite(v.w);
        if (filtered) u = v;
    }
    DenoisePixel o;
    o.u = u;
    o.pos = make_float4(p.x, p.y, p.z, filtered ? 1.0f : 0.0f);
    o.nrm = make_float4(nn.x, nn.y, nn.z, 0.0f);
    o.albedo = make_float4(a[0], a[1], a[2], 0.0f);
    o.rgb = make_float4(c[0], c[1], c[2], 0.0f);
    DenoisePixel *dst = reinterpret_cast<DenoisePixel *>(out);
    dst[i] = o;
}
void launch_denoise_prepare(const StripDev &st, const float *rgb, const float *var, const float4 *pos, const float4 *nrm, const float4 *dif,
                            const float4 *phg, const float4 *light, float4 *out, hipStream_t s) {
    const size_t n = (size_t)st.W * st.local_rows;
    if (n == 0) return;
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, st, rgb, var, pos, nrm, dif, phg, light, out);
}

// One a-trous pass at step h over a frame of W x rows packed pixels (rows from the bottom).  in: (u, s) of every pixel, `in_step` float4
// apart (the packed frame for the first pass, a plane after it); out: (u', s') of every pixel, a plane.  A pixel that is not filtered is
// copied and is never a tap.  16 x 16 pixels per workgroup (a wave covers 16 x 4): the taps of neighbouring lanes fall on the same lines.
__global__ __launch_bounds__(256) void denoise_level_kernel(DenoiseLevelArgs a) {
    const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
    if (x >= a.W || y >= a.rows) return;
    const size_t i = (size_t)y * a.W + x;
    const DenoisePixel *g = a.frame;
    const float4 up = a.in[i * a.in_step];
    if (g[i].pos.w == 0.0f) { a.out[i] = up; return; }
    const float4 xp = g[i].pos, np = g[i].nrm;
    // g_p: this pass's s blurred over the 3 x 3 filtered neighbours, [1/4, 1/2, 1/4]^2, normalised by the weights used
    const float b3[3] = { 0.25f, 0.5f, 0.25f };
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; dy++) {
        const int qy = y + dy;
        if (qy < 0 || qy >= a.rows) continue;
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx;
            if (qx < 0 || qx >= a.W) continue;
            const size_t q = (size_t)qy * a.W + qx;
            if (g[q].pos.w == 0.0f) continue;
            const float k = b3[dx + 1] * b3[dy + 1];
            gs = gs + k * a.in[q * a.in_step].w;
            gw = gw + k;
        }
    }
    const float gp = gs / gw;
    const float lp = luminance(up.x, up.y, up.z);
    const float dl = a.sigma_l * sqrtf(gp) + 1e-10f;
    const float b5[5] = { 1.0f / 16.0f, 0.25f, 0.375f, 0.25f, 1.0f / 16.0f };
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, ss = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + a.h * dy;
        if (qy < 0 || qy >= a.rows) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + a.h * dx;
            if (qx < 0 || qx >= a.W) continue;
            const size_t q = (size_t)qy * a.W + qx;
            const float4 xq = g[q].pos;
            if (xq.w == 0.0f) continue;
            const float4 nq = g[q].nrm, uq = a.in[q * a.in_step];
            const float k = b5[dx + 2] * b5[dy + 2];
            const float el = fabsf(lp - luminance(uq.x, uq.y, uq.z)) / dl;
            const float ex = fabsf((np.x * (xq.x - xp.x) + np.y * (xq.y - xp.y)) + np.z * (xq.z - xp.z)) / a.sigma_x_r;
            const float nd = fmaxf(0.0f, (np.x * nq.x + np.y * nq.y) + np.z * nq.z);
            const float w = (k * expf(-el - ex)) * powf(nd, a.sigma_n);
            sw = sw + w;
            sr = sr + w * uq.x; sg = sg + w * uq.y; sb = sb + w * uq.z;
            ss = ss + (w * w) * uq.w;
        }
    }
    // (the centre tap has weight k(0, 0) |n_p|^(2 sigma_n) > 0 for a unit normal; a degenerate normal keeps the pixel as it is)
    if (!(sw > 0.0f)) { a.out[i] = up; return; }
    a.out[i] = make_float4(sr / sw, sg / sw, sb / sw, ss / (sw * sw));
}
void launch_denoise_level(const DenoiseLevelArgs &a, hipStream_t s) {
    if (a.W <= 0 || a.rows <= 0) return;
    hipLaunchKernelGGL(denoise_level_kernel, dim3((unsigned)((a.W + 15) / 16), (unsigned)((a.rows + 15) / 16)), dim3(256), 0, s, a);
}

// out (3 floats per pixel, resolve's layout): albedo * u for a filtered pixel (its light plane is zero: the light term adds nothing), the
// composite for every other pixel, bit for bit
__global__ __launch_bounds__(256) void denoise_finish_kernel(const DenoisePixel *frame, const float4 *u, size_t n, float *out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const DenoisePixel &p = frame[i];
    float r = p.rgb.x, g = p.rgb.y, b = p.rgb.z;
    if (p.pos.w != 0.0f) { const float4 v = u[i]; r = p.albedo.x * v.x; g = p.albedo.y * v.y; b = p.albedo.z * v.z; }
    out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
}
void launch_denoise_finish(const DenoisePixel *frame, const float4 *u, size_t n, float *out_rgb, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(denoise_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, frame, u, n, out_rgb);
}

} // namespace evplp
