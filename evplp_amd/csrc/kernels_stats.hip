// The statistics kernels: evplp_frame_error, evplp_noise_* (fold, shard pooling, estimate, variance image), evplp_adaptive_retire,
// evplp_adaptive_tile_noise and budget mode's per-tile fold.  Tests restate every operation of theirs in numpy, so the unit is built with
// -ffp-contract=off (Makefile) and every operation that matters is an _rn intrinsic.  Each family has ONE body: a plain kernel and its
// *_frozen variant (retired tiles, AdaptTiles) are the two instances of one template.
#include "device_common.hpp"
#include "kernels.h"

namespace evplp {

// ---- the noise tracker's per-pixel arithmetic
// the record of the 8 x 8 tile that holds pixel (x, local row l)
EV_DEV int4 tile_record(const AdaptTiles &at, int l, int x) { return at.tiles[(l >> 3) * at.tiles_x + (x >> 3)]; }
// Q and S of pixel i, per channel
__device__ inline void noise_moments(const NoiseMoments &m, size_t i, double q[3], double s[3]) {
    for (int ch = 0; ch < 3; ch++) q[ch] = m.q[ch * m.stride + i];
    if (m.s) { for (int ch = 0; ch < 3; ch++) s[ch] = m.s[ch * m.stride + i]; return; }
    const float4 a = m.prev[i], b = m.start[i];
    s[0] = (double)__fsub_rn(a.x, b.x); s[1] = (double)__fsub_rn(a.y, b.y); s[2] = (double)__fsub_rn(a.z, b.z);
}
// v = (Q - S * S / K) / (B - 1) of one channel, before the clamp: not finite when a sum of the pixel is not (Inf - Inf, NaN) or overflowed
__device__ inline double noise_v(double q, double s, double K, double B1) { return __ddiv_rn(__dsub_rn(q, __ddiv_rn(__dmul_rn(s, s), K)), B1); }
// the variance of one channel of the image scale * c: s2K * max(0, v), s2K = scale^2 * K.  A NaN v reads 0 (the comparison is false) and
// +Inf stays: evplp_noise_variance's bytes (include/evplp.h), which the denoiser reads.
__device__ inline double noise_var_of(double v, double s2K) { return __dmul_rn(s2K, v > 0.0 ? v : 0.0); }
__device__ inline double noise_var(double q, double s, double K, double B1, double s2K) { return noise_var_of(noise_v(q, s, K, B1), s2K); }
// the variance of one channel of a RETIRED pixel (tile record r): the tracker's figure at retirement, rescaled to today's composite --
// noise_var(Q, S, K_t, B_t - 1, s2K_t), s2K_t = ((scale * N) / n_t)^2 * K_t
__device__ inline double noise_var_retired(double q, double s, const int4 &r, const AdaptTiles &at) {
    const double f = __ddiv_rn(__dmul_rn(at.scale, at.n), (double)r.x);
    return noise_var(q, s, (double)r.y, (double)r.z - 1.0, __dmul_rn(__dmul_rn(f, f), (double)r.y));
}
// num of pixel (x, local row l) from its moments (its tile's record: Adapt only): (var_r + var_g) + var_b, fp64.  sound = every channel's
// v is finite (the retired form's v for a retired pixel), tested before the clamp and the s2K factor: the clamp would read a NaN v as 0
template <bool Adapt>
__device__ inline double noise_num(const double q[3], const double sm[3], double K, double B1, double s2K, const AdaptTiles &at, int l, int x, bool &sound) {
    if constexpr (Adapt) {
        const int4 r = tile_record(at, l, x);
        if (r.x != 0) {
            const double f = __ddiv_rn(__dmul_rn(at.scale, at.n), (double)r.x);
            K = (double)r.y; B1 = (double)r.z - 1.0; s2K = __dmul_rn(__dmul_rn(f, f), (double)r.y);      // (noise_var_retired)
        }
    }
    const double v0 = noise_v(q[0], sm[0], K, B1), v1 = noise_v(q[1], sm[1], K, B1), v2 = noise_v(q[2], sm[2], K, B1);
    sound = isfinite(v0) && isfinite(v1) && isfinite(v2);
    return __dadd_rn(__dadd_rn(noise_var_of(v0, s2K), noise_var_of(v1, s2K)), noise_var_of(v2, s2K));
}
// A tile's rel, summed: lane = pixel (x, local row l).  The lane forms noise_rows_kernel's rel (0 outside the image, and 0 for a broken pixel:
// a decision works around the break); the sum over the 64 lanes is a fixed tree (shuffle-down by 32, 16, .. 1) and so is the count of sound
// in-image pixels; every lane returns lane 0's pair.
template <bool Adapt>
__device__ __forceinline__ void tile_rel_sum(const StripDev &st, const NoiseMoments &m, double K, double B1, double s2K, const float4 *light, float ls,
                                             int mask_emitter, const float *rgb, const AdaptTiles &at, int x, int l, double &rel, double &cnt) {
    const bool in = x < st.W && l < st.local_rows && st.global_row(l) < st.H;
    rel = 0.0; cnt = 0.0;
    if (in) {
        const size_t i = (size_t)l * st.W + x;
        double num = 0.0;
        bool sound = true;
        if (!(mask_emitter && 0.0f < __fmul_rn(light[i].x, ls))) {
            double q[3], sm[3];
            noise_moments(m, i, q, sm);
            num = noise_num<Adapt>(q, sm, K, B1, s2K, at, l, x, sound);
        }
        const double r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        const double den = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(r, r), __dmul_rn(g, g)), __dmul_rn(b, b)), 0.001);
        if (sound && isfinite(den)) { rel = __ddiv_rn(num, den); cnt = 1.0; }       // (a broken pixel adds nothing and is not counted)
    }
    for (int off = 32; off > 0; off >>= 1) { rel = __dadd_rn(rel, __shfl_down(rel, off, 64)); cnt = __dadd_rn(cnt, __shfl_down(cnt, off, 64)); }
    rel = __shfl(rel, 0, 64); cnt = __shfl(cnt, 0, 64);
}

// ---- one image row's four fp64 sums (frame_error_kernel, noise_rows_body): a workgroup of kRowThreads per local row l, thread t takes the
// pixels t, t + 256, .. of the row in increasing x into its s[4].  The sum has a fixed shape: each wave folds its lanes by a fixed shuffle
// tree, and thread 0 adds the four waves in order.  A row's figures are a function of the row alone -- not of the rank that holds it, nor
// of its local row -- and nothing is atomic; the host adds the rows in image order (evplp::sum_row_errors).
constexpr int kRowThreads = 256;
EV_DEV void reduce_row(double s[4], int l, RowError *rows) {
    __shared__ double wave_sums[kRowThreads / 64][4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_down(s[k], off, 64);
    if (lane == 0) for (int k = 0; k < 4; k++) wave_sums[wave][k] = s[k];
    __syncthreads();
    if (tid == 0) {
        double t[4];
        for (int k = 0; k < 4; k++) {
            t[k] = wave_sums[0][k];
            for (int w = 1; w < kRowThreads / 64; w++) t[k] += wave_sums[w][k];
        }
        rows[l] = RowError{ t[0], t[1], t[2], t[3] };
    }
}

// evplp_frame_error: the composite against a reference image, one workgroup per local row (reduce_row).  The per-pixel terms are fp32 in the
// order of floatimage.cpp:64-112 -- d = img - ref, num = d.x^2 + d.y^2 + d.z^2, den = |ref|^2 + 0.001, rel = num / den -- every operation
// rounded on its own (no contraction, a correctly rounded division), so that numpy's float32 reproduces every term.  They are summed in fp64.
__global__ __launch_bounds__(kRowThreads) void frame_error_kernel(StripDev st, const float *rgb, const float *ref, const uint8_t *keep, RowError *rows) {
    const int l = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int y = st.global_row(l);
    double s[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (y < st.H) {
        const size_t own = (size_t)l * st.W, top = (size_t)(st.H - 1 - y) * st.W;     // (the reference's rows run top to bottom)
        for (int x = tid; x < st.W; x += kRowThreads) {
            const float *a = rgb + 3 * (own + x), *r = ref + 3 * (top + x);
            const float rx = r[0], ry = r[1], rz = r[2];
            const float dx = __fsub_rn(a[0], rx), dy = __fsub_rn(a[1], ry), dz = __fsub_rn(a[2], rz);
            const float num = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            const float den = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry)), __fmul_rn(rz, rz)), 0.001f);
            const float rel = __fdiv_rn(num, den);
            s[0] += (double)num; s[1] += (double)rel;
            if (!keep || keep[top + x]) { s[2] += (double)rel; s[3] += 1.0; }
        }
    }
    reduce_row(s, l, rows);
}
void launch_frame_error(const StripDev &st, const float *rgb, const float *ref, const uint8_t *keep, RowError *rows, hipStream_t s) {
    if (st.local_rows <= 0) return;
    hipLaunchKernelGGL(frame_error_kernel, dim3((unsigned)st.local_rows), dim3(kRowThreads), 0, s, st, rgb, ref, keep, rows);
}

// ---- per-pixel noise from the running sums (include/evplp.h evplp_noise_*).
// Fold: thread t takes the pixels 2t and 2t + 1 -- the accumulator and c_prev planes as float4, Q as one double2 per channel plane (its
// planes are padded to an even pixel count, so the pair's load never leaves them).  Per channel, fp32: c = vpl + photon, d = c - c_prev;
// fp64: Q += d * d / k.  Init (k = 0): c_prev = c_start = c, Q = 0.  One pass, no atomics: 112 B per pixel.
// (n = W * local_rows, and every context's local_rows is a multiple of 8: n is even for every caller today, so the lone last pixel,
// two == false, is a guard that no entry point reaches and no test runs.)
// Adapt (evplp_adaptive_retire): a pixel of a retired tile keeps its Q and c_prev (its sum grows by the same extrapolated step every
// iteration; folded, that would look like a pixel without noise).
EV_DEV bool pixel_retired(const AdaptTiles &at, int W, size_t i) {
    const int ly = (int)(i / (size_t)W), x = (int)(i - (size_t)ly * W);
    return tile_record(at, ly, x).x != 0;
}
template <bool Init, bool Adapt>
__device__ __forceinline__ void noise_fold_body(NoisePlanes m, const float4 *vpl, const float4 *pm, size_t n, double k, AdaptTiles at, int W) {
    const size_t i = 2 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const bool two = i + 1 < n;
    float4 c[2];
    for (int j = 0; j < 2; j++) {
        if (j == 1 && !two) { c[1] = make_float4(0.f, 0.f, 0.f, 0.f); break; }
        const float4 v = vpl[i + j], p = pm[i + j];
        c[j] = make_float4(__fadd_rn(v.x, p.x), __fadd_rn(v.y, p.y), __fadd_rn(v.z, p.z), 0.f);
    }
    if (Init) {
        for (int j = 0; j < (two ? 2 : 1); j++) { m.prev[i + j] = c[j]; m.start[i + j] = c[j]; }
        for (int ch = 0; ch < 3; ch++) *(double2 *)(m.q + ch * m.stride + i) = make_double2(0.0, 0.0);
        return;
    }
    float4 prev[2];
    prev[0] = m.prev[i]; prev[1] = two ? m.prev[i + 1] : make_float4(0.f, 0.f, 0.f, 0.f);
    double2 q[3];
    for (int ch = 0; ch < 3; ch++) q[ch] = *(const double2 *)(m.q + ch * m.stride + i);
    double d[2][3];
    for (int j = 0; j < 2; j++) {
        d[j][0] = (double)__fsub_rn(c[j].x, prev[j].x); d[j][1] = (double)__fsub_rn(c[j].y, prev[j].y); d[j][2] = (double)__fsub_rn(c[j].z, prev[j].z);
    }
    bool frozen[2] = { false, false };
    double2 q0[3];
    if constexpr (Adapt) {
        frozen[0] = pixel_retired(at, W, i); frozen[1] = two && pixel_retired(at, W, i + 1);
        for (int ch = 0; ch < 3; ch++) q0[ch] = q[ch];
    }
    for (int ch = 0; ch < 3; ch++) {
        q[ch].x = __dadd_rn(q[ch].x, __ddiv_rn(__dmul_rn(d[0][ch], d[0][ch]), k));
        q[ch].y = __dadd_rn(q[ch].y, __ddiv_rn(__dmul_rn(d[1][ch], d[1][ch]), k));      // (a lone last pixel: the pad gains 0)
        if constexpr (Adapt) { if (frozen[0]) q[ch].x = q0[ch].x; if (frozen[1]) q[ch].y = q0[ch].y; }
        *(double2 *)(m.q + ch * m.stride + i) = q[ch];
    }
    if (!frozen[0]) m.prev[i] = c[0];
    if (two && !frozen[1]) m.prev[i + 1] = c[1];
}
template <bool Init>
__global__ __launch_bounds__(256) void noise_fold_kernel(NoisePlanes m, const float4 *vpl, const float4 *pm, size_t n, double k) {
    noise_fold_body<Init, false>(m, vpl, pm, n, k, AdaptTiles{}, 0);
}
__global__ __launch_bounds__(256) void noise_fold_frozen_kernel(NoisePlanes m, const float4 *vpl, const float4 *pm, size_t n, double k, AdaptTiles at, int W) {
    noise_fold_body<false, true>(m, vpl, pm, n, k, at, W);
}
void launch_noise_fold(const NoisePlanes &m, const float4 *vpl, const float4 *pm, const StripDev &st, const AdaptTiles &at, int32_t k, hipStream_t s) {
    const size_t n = (size_t)st.W * st.local_rows, threads = (n + 1) / 2;
    if (threads == 0) return;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (k == 0) hipLaunchKernelGGL(noise_fold_kernel<true>, grid, dim3(256), 0, s, m, vpl, pm, n, 1.0);
    else if (!at.tiles) hipLaunchKernelGGL(noise_fold_kernel<false>, grid, dim3(256), 0, s, m, vpl, pm, n, (double)k);
    else hipLaunchKernelGGL(noise_fold_frozen_kernel, grid, dim3(256), 0, s, m, vpl, pm, n, (double)k, at, st.W);
}

// evplp_noise_fold in budget mode: one wavefront per tile of the planes, lane = pixel.  The record is read once, wave-uniform, and written by
// lane 0 after the tile's pixels: nobody else touches the tile, so the element-wise pass and the record update cannot race.
__global__ __launch_bounds__(64) void noise_fold_budget_kernel(NoisePlanes m, StripDev st, int4 *tiles, const float4 *snap) {
    const int tile = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int nt = __builtin_amdgcn_readfirstlane(tiles[tile].x), kt = __builtin_amdgcn_readfirstlane(tiles[tile].y);
    const int bt = __builtin_amdgcn_readfirstlane(tiles[tile].z), budget = __builtin_amdgcn_readfirstlane(tiles[tile].w);
    if (nt == kt) return;
    const double k = (double)(nt - kt);
    const int2 xl = tile_lane(tile, lane, st.W);
    const int x = xl.x, l = xl.y;
    if (x < st.W && l < st.local_rows) {
        const size_t i = (size_t)l * st.W + x;
        const float4 R = snap[i], prev = m.prev[i];
        const double d[3] = { (double)__fsub_rn(R.x, prev.x), (double)__fsub_rn(R.y, prev.y), (double)__fsub_rn(R.z, prev.z) };
        for (int ch = 0; ch < 3; ch++) {
            double *q = m.q + ch * m.stride + i;
            *q = __dadd_rn(*q, __ddiv_rn(__dmul_rn(d[ch], d[ch]), k));
        }
        m.prev[i] = make_float4(R.x, R.y, R.z, 0.f);
    }
    if (lane == 0) tiles[tile] = make_int4(nt, nt, bt + 1, budget);
}
void launch_noise_fold_budget(const NoisePlanes &m, const StripDev &st, int4 *tiles, const float4 *snap, int32_t ntiles, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(noise_fold_budget_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, m, st, tiles, snap);
}

// Shard pooling (EVPLP_PARTITION_ITERATIONS): launched once per shard in rank order; q / s_out = first ? the shard's : + the shard's
__global__ __launch_bounds__(256) void noise_pool_kernel(NoiseMoments src, int first, double *q, double *s_out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double qs[3], ss[3];
    noise_moments(src, i, qs, ss);
    for (int ch = 0; ch < 3; ch++) {
        const size_t o = ch * src.stride + i;
        q[o] = first ? qs[ch] : __dadd_rn(q[o], qs[ch]);
        s_out[o] = first ? ss[ch] : __dadd_rn(s_out[o], ss[ch]);
    }
}
void launch_noise_pool(const NoiseMoments &src, bool first, double *q, double *s_out, size_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(noise_pool_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, first ? 1 : 0, q, s_out, n);
}

// evplp_noise_estimate: one workgroup per local row, the reduction of frame_error_kernel (reduce_row).  Per pixel, fp64:
// var_ch = noise_var(..) (0 on an emitter pixel under mask_emitter: 0 < light.x * ls), num = (var_r + var_g) + var_b,
// den = ((r * r + g * g) + b * b) + 0.001 of the composite, rel = num / den.  A broken pixel (include/evplp.h evplp_noise_track: den or one
// of its three v not finite) has num = rel = NaN: the figures it enters say that they are broken.
// Adapt: retired pixels with noise_var_retired (noise_num)
template <bool Adapt>
__device__ __forceinline__ void noise_rows_body(StripDev st, NoiseMoments m, double K, double B1, double s2K, const float4 *light,
                                                float ls, int mask_emitter, const float *rgb, const uint8_t *keep, RowError *rows, AdaptTiles at) {
    const int l = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int y = st.global_row(l);
    double s[4] = { 0.0, 0.0, 0.0, 0.0 };
    if (y < st.H) {
        const size_t own = (size_t)l * st.W, top = (size_t)(st.H - 1 - y) * st.W;     // (the mask's rows run top to bottom)
        for (int x = tid; x < st.W; x += kRowThreads) {
            const size_t i = own + x;
            double num = 0.0;
            bool sound = true;
            if (!(mask_emitter && 0.0f < __fmul_rn(light[i].x, ls))) {
                double q[3], sm[3];
                noise_moments(m, i, q, sm);
                num = noise_num<Adapt>(q, sm, K, B1, s2K, at, l, x, sound);
            }
            const double r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
            const double den = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(r, r), __dmul_rn(g, g)), __dmul_rn(b, b)), 0.001);
            if (!(sound && isfinite(den))) num = __builtin_nan("");                 // (a broken pixel says so: num and rel are NaN)
            const double rel = __ddiv_rn(num, den);
            s[0] += num; s[1] += rel;
            if (!keep || keep[top + x]) { s[2] += rel; s[3] += 1.0; }
        }
    }
    reduce_row(s, l, rows);
}
__global__ __launch_bounds__(kRowThreads) void noise_rows_kernel(StripDev st, NoiseMoments m, double K, double B1, double s2K, const float4 *light,
                                                                  float ls, int mask_emitter, const float *rgb, const uint8_t *keep, RowError *rows) {
    noise_rows_body<false>(st, m, K, B1, s2K, light, ls, mask_emitter, rgb, keep, rows, AdaptTiles{});
}
__global__ __launch_bounds__(kRowThreads) void noise_rows_frozen_kernel(StripDev st, NoiseMoments m, double K, double B1, double s2K, const float4 *light,
                                                                         float ls, int mask_emitter, const float *rgb, const uint8_t *keep, RowError *rows, AdaptTiles at) {
    noise_rows_body<true>(st, m, K, B1, s2K, light, ls, mask_emitter, rgb, keep, rows, at);
}
void launch_noise_rows(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, const float4 *light, float ls, int mask_emitter,
                       const float *rgb, const uint8_t *keep, RowError *rows, const AdaptTiles &at, hipStream_t s) {
    if (st.local_rows <= 0) return;
    const dim3 grid((unsigned)st.local_rows), block(kRowThreads);
    if (!at.tiles) hipLaunchKernelGGL(noise_rows_kernel, grid, block, 0, s, st, m, K, B - 1.0, s2K, light, ls, mask_emitter, rgb, keep, rows);
    else hipLaunchKernelGGL(noise_rows_frozen_kernel, grid, block, 0, s, st, m, K, B - 1.0, s2K, light, ls, mask_emitter, rgb, keep, rows, at);
}

// evplp_noise_variance: (float) noise_var per channel of every plane pixel
// (Adapt: retired pixels with noise_var_retired)
template <bool Adapt>
__device__ __forceinline__ void noise_variance_body(NoiseMoments m, double K, double B1, double s2K, size_t n, float *out, AdaptTiles at, int W) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double q[3], s[3];
    noise_moments(m, i, q, s);
    if constexpr (Adapt) {
        const int ly = (int)(i / (size_t)W), x = (int)(i - (size_t)ly * W);
        const int4 r = tile_record(at, ly, x);
        if (r.x != 0) { for (int ch = 0; ch < 3; ch++) out[3 * i + ch] = (float)noise_var_retired(q[ch], s[ch], r, at); return; }
    }
    for (int ch = 0; ch < 3; ch++) out[3 * i + ch] = (float)noise_var(q[ch], s[ch], K, B1, s2K);
}
__global__ __launch_bounds__(256) void noise_variance_kernel(NoiseMoments m, double K, double B1, double s2K, size_t n, float *out) {
    noise_variance_body<false>(m, K, B1, s2K, n, out, AdaptTiles{}, 0);
}
__global__ __launch_bounds__(256) void noise_variance_frozen_kernel(NoiseMoments m, double K, double B1, double s2K, size_t n, float *out, AdaptTiles at, int W) {
    noise_variance_body<true>(m, K, B1, s2K, n, out, at, W);
}
void launch_noise_variance(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, float *out_rgb, const AdaptTiles &at, hipStream_t s) {
    const size_t n = (size_t)st.W * st.local_rows;
    if (n == 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (!at.tiles) hipLaunchKernelGGL(noise_variance_kernel, grid, dim3(256), 0, s, m, K, B - 1.0, s2K, n, out_rgb);
    else hipLaunchKernelGGL(noise_variance_frozen_kernel, grid, dim3(256), 0, s, m, K, B - 1.0, s2K, n, out_rgb, at, st.W);
}

// evplp_adaptive_retire: one wavefront per tile of the context's planes, lane = pixel (x = 8 tx + lane % 8, local row 8 ty + lane / 8).  An
// active tile's lanes form noise_rows_kernel's rel (0 outside the image); the sum over the 64 lanes is a fixed tree (shuffle-down by 32, 16,
// .. 1: lane 0 holds it), so is the count of sound in-image pixels, and mean = sum / count in fp64.  mean <= tau (and a sound pixel): the
// record becomes { n, K, B, 0 } and every plane pixel of the tile copies its VPL_ACCUM into the snapshot.  A tile retired before is left
// alone.  The decision is the wavefront's own: no atomics.
__global__ __launch_bounds__(64) void adaptive_retire_kernel(StripDev st, NoiseMoments m, double K, double B1, double s2K, const float4 *light, float ls,
                                                            int mask_emitter, const float *rgb, double tau, int4 *tiles, int tiles_x, int n, int ki, int bi,
                                                            const float4 *vpl, float4 *snap) {
    const int tile = (int)blockIdx.x, tx = tile % tiles_x, ty = tile / tiles_x;
    if (__builtin_amdgcn_readfirstlane(tiles[tile].x) != 0) return;
    const int lane = (int)threadIdx.x, x = tx * 8 + (lane & 7), l = ty * 8 + (lane >> 3);
    const bool plane = x < st.W && l < st.local_rows;
    double rel, cnt;
    tile_rel_sum<false>(st, m, K, B1, s2K, light, ls, mask_emitter, rgb, AdaptTiles{}, x, l, rel, cnt);
    if (!(cnt > 0.0) || !(__ddiv_rn(rel, cnt) <= tau)) return;
    if (plane) snap[(size_t)l * st.W + x] = vpl[(size_t)l * st.W + x];
    if (lane == 0) tiles[tile] = make_int4(n, ki, bi, 0);
}
void launch_adaptive_retire(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, const float4 *light, float ls, int mask_emitter,
                            const float *rgb, double tau, int4 *tiles, int32_t tiles_x, int32_t tiles_y, int32_t n, const float4 *vpl, float4 *snap, hipStream_t s) {
    if (tiles_x <= 0 || tiles_y <= 0) return;
    hipLaunchKernelGGL(adaptive_retire_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(64), 0, s, st, m, K, B - 1.0, s2K, light, ls, mask_emitter, rgb, tau,
                       tiles, tiles_x, n, (int)K, (int)B, vpl, snap);
}

// evplp_adaptive_tile_noise, one wavefront per tile of the planes: adaptive_retire_kernel's per-tile mean (tile_rel_sum), written out instead
// of compared; a tile with a record (retired, or any tile of budget mode) is priced with noise_var_retired
__global__ __launch_bounds__(64) void tile_noise_kernel(StripDev st, NoiseMoments m, double K, double B1, double s2K, const float4 *light, float ls,
                                                       int mask_emitter, const float *rgb, AdaptTiles at, double *out) {
    const int tile = (int)blockIdx.x, tx = tile % at.tiles_x, ty = tile / at.tiles_x;
    const int lane = (int)threadIdx.x, x = tx * 8 + (lane & 7), l = ty * 8 + (lane >> 3);
    double rel, cnt;
    tile_rel_sum<true>(st, m, K, B1, s2K, light, ls, mask_emitter, rgb, at, x, l, rel, cnt);
    if (lane == 0) out[tile] = cnt > 0.0 ? __ddiv_rn(rel, cnt) : 0.0;
}
void launch_tile_noise(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, const float4 *light, float ls, int mask_emitter,
                       const float *rgb, const AdaptTiles &at, int32_t ntiles, double *out, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(tile_noise_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, st, m, K, B - 1.0, s2K, light, ls, mask_emitter, rgb, at, out);
}

} // namespace evplp
