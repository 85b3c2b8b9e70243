// Lightmap baking (evplp_surface_points, evplp_lightmap_samples, evplp_bake_lightmap; lightmap.cpp): from a hit to the G-buffer's four
// float4, from an atlas texel to a hit, and from a band's gathered samples to its texels.
//   lightmap_points_kernel  <- lane = hit: primary_body.hpp's hit point, flat winding normal and material_at, operation for operation; the
//                              unit is built without contraction as the feeders are, so a point carries the G-buffer's bits
//   lightmap_setup_kernel   <- lane = triangle of the selection: the snap and the orientation of lightmap_raster.h, once per call
//   lightmap_count_kernel   <- lane = triangle: the 8 x 8-texel tiles of the band its snapped box touches and no edge excludes, integer atomics
//   lightmap_fill_kernel    <- the same walk again, behind the exclusive sum of the counts (hipCUB): the tiles' triangle lists
//   lightmap_raster_kernel  <- one wave per tile, lane = texel.  The tile's list goes through LDS 64 triangles at a time: each lane sets one
//                              triangle's three edge functions up (E = dx py - dy px + c, the ownership rule folded into c), then every lane
//                              tests all of them at its S x S samples with 64-bit adds.  A sample keeps the LOWEST index that covers it, so
//                              the order in which the atomics filled the list cannot change a byte of the result.
//   lightmap_resolve_kernel <- lane = texel of a band: the fp32 sums over its valid samples in ascending (j, i), divided by their count
//   lightmap_gutter_kernel  <- lane = texel of the atlas: one dilation pass, reading the state before it
// No float atomics anywhere; nothing here is shared with another kernel unit's code object.
#include "device_common.hpp"
#include "kernels.h"
#include "lightmap.hpp"

#include <hipcub/hipcub.hpp>

namespace evplp {

namespace {
EV_DEV bool lm_finite(float x) { return fabsf(x) <= 3.4028235e38f; }        // (false for a NaN)
EV_DEV bool lm_finite(V3 x) { return lm_finite(x.x) && lm_finite(x.y) && lm_finite(x.z); }

// a triangle as the raster kernel's lanes read it from LDS: E_k(px, py) = dx[k] py - dy[k] px + c[k] >= 0 for k = 0, 1, 2 is the inside test
struct LmStaged { int32_t dx[3], dy[3]; int64_t c[3]; uint32_t index; uint32_t pad; };
static_assert(sizeof(LmStaged) == 56, "three edges and the index");

EV_DEV void lm_stage(const lm_tri &t, uint32_t index, LmStaged &q) {
    const int32_t *v = t.v;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int32_t ax = v[2 * k], ay = v[2 * k + 1], bx = v[(2 * k + 2) % 6], by = v[(2 * k + 3) % 6];
        const int32_t dx = bx - ax, dy = by - ay;
        q.dx[k] = dx; q.dy[k] = dy;
        // (bx - ax)(py - ay) - (by - ay)(px - ax) = dx py - dy px + (dy ax - dx ay); E > 0 || (E == 0 && own)  <=>  E - (own ? 0 : 1) >= 0
        q.c[k] = (int64_t)dy * (int64_t)ax - (int64_t)dx * (int64_t)ay - (lm_owns(dx, dy) ? 0 : 1);
    }
    q.index = index; q.pad = 0u;
}

// the tiles of the band that triangle k of the selection may cover: its snapped box in texels, clipped by the atlas and the band, and of
// those tiles the ones no edge excludes (the largest value of an edge function over the tile's samples is negative).  The count and the
// fill walk the same tiles: f(tile) is called once for each.
template <typename F> EV_DEV void lm_for_each_tile(const RasterArgs &a, const lm_tri &t, F f) {
    if (!(t.flags & LM_TRI_VALID)) return;
    const int32_t *v = t.v;
    const int32_t minx = min(v[0], min(v[2], v[4])), maxx = max(v[0], max(v[2], v[4])), miny = min(v[1], min(v[3], v[5])), maxy = max(v[1], max(v[3], v[5]));
    // (>> of a negative number is an arithmetic shift: floor)
    const int32_t x_lo = max(minx >> LM_SUB_BITS, 0), x_hi = min(maxx >> LM_SUB_BITS, a.width - 1);
    const int32_t y_lo = max(miny >> LM_SUB_BITS, a.y0), y_hi = min(maxy >> LM_SUB_BITS, a.y0 + a.rows - 1);
    if (x_lo > x_hi || y_lo > y_hi) return;
    LmStaged q; lm_stage(t, 0u, q);
    for (int32_t ty = (y_lo - a.y0) >> 3; ty <= (y_hi - a.y0) >> 3; ty++) {
        const int32_t py_lo = LM_SUB * (a.y0 + 8 * ty), py_hi = py_lo + 8 * LM_SUB;           // the tile's samples lie strictly inside
        for (int32_t tx = x_lo >> 3; tx <= x_hi >> 3; tx++) {
            const int32_t px_lo = LM_SUB * 8 * tx, px_hi = px_lo + 8 * LM_SUB;
            bool out = false;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int64_t e = (int64_t)q.dx[k] * (int64_t)(q.dx[k] >= 0 ? py_hi : py_lo) - (int64_t)q.dy[k] * (int64_t)(q.dy[k] >= 0 ? px_lo : px_hi) + q.c[k];
                out |= e < 0;
            }
            if (!out) f((uint32_t)(ty * a.tiles_x + tx));
        }
    }
}
}

__global__ __launch_bounds__(256) void lightmap_points_kernel(PointsArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.n) return;
    const float4 h = reinterpret_cast<const float4 *>(a.hits)[i];
    const float b = h.y, g = h.z;                               // (t is not read)
    const int32_t tri = __float_as_int(h.w);
    float4 pos = make_float4(0.f, 0.f, 0.f, 0.f), nrm = pos, dif = pos, phg = pos;
    if (tri >= 0 && tri < a.ntris && lm_finite(b) && lm_finite(g)) {
        // primary_body.hpp, the hit's four texels
        const TriAttr &ta = a.sc.attrs[tri];
        V3 p0 = v3(ta.v), p1 = v3(ta.v + 3), p2 = v3(ta.v + 6);
        const float w0 = 1.0f - b - g;
        V3 P = v3((p1.x * b + p2.x * g) + p0.x * w0, (p1.y * b + p2.y * g) + p0.y * w0, (p1.z * b + p2.z * g) + p0.z * w0);
        V3 N = normalize_exact(cross_exact(p1 - p0, p2 - p0));
        if (lm_finite(N)) {                                     // (a triangle without area has none)
            V3 kd = v3(1.f, 1.f, 1.f), ks = v3(0.f, 0.f, 0.f); float ns = 0.0f;
            if (!(a.flags & EVPLP_POINTS_WHITE)) material_at(a.sc, ta, b, g, kd, ks, ns);
            if (a.flags & EVPLP_POINTS_FACE_EYES) {
                const float *e = a.eyes + 3 * (size_t)i;
                if (dot_exact(N, v3(e[0], e[1], e[2]) - P) < 0.0f) N = -N;
            }
            pos = make_float4(P.x, P.y, P.z, 1.0f);
            nrm = make_float4(N.x, N.y, N.z, 0.f);
            dif = make_float4(kd.x, kd.y, kd.z, 0.f);
            phg = make_float4(ks.x, ks.y, ks.z, ns);
        }
    }
    float4 *o = a.out + 4 * (size_t)i;
    o[0] = pos; o[1] = nrm; o[2] = dif; o[3] = phg;
}

__global__ __launch_bounds__(256) void lightmap_setup_kernel(RasterArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (uint32_t)a.count) return;
    float uv[6];
    const float *src = a.uvs ? a.uvs + 6 * (size_t)k : a.attrs[(size_t)a.first + k].uv;
#pragma unroll
    for (int j = 0; j < 6; j++) uv[j] = src[j];
    lm_tri t;
    lm_setup(uv, a.width, a.height, &t);
    a.tris[k] = t;
}

__global__ __launch_bounds__(256) void lightmap_count_kernel(RasterArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (uint32_t)a.count) return;
    lm_for_each_tile(a, a.tris[k], [&](uint32_t tile) { atomicAdd(&a.counts[tile], 1u); });
}

__global__ __launch_bounds__(256) void lightmap_fill_kernel(RasterArgs a) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= (uint32_t)a.count) return;
    lm_for_each_tile(a, a.tris[k], [&](uint32_t tile) {
        const uint32_t slot = a.offsets[tile] + atomicAdd(&a.cursors[tile], 1u);
        if (slot < a.offsets[tile + 1] && slot < a.pairs) a.list[slot] = k;
    });
}

template <int S> __global__ __launch_bounds__(64) void lightmap_raster_kernel(RasterArgs a) {
    __shared__ LmStaged staged[64];
    const int tile = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;          // wave-uniform
    const int32_t x = tx * 8 + (lane & 7), yl = ty * 8 + (lane >> 3);
    const bool live = x < a.width && yl < a.rows;
    const int32_t px0 = lm_sample(x, 0, S), py0 = lm_sample(a.y0 + yl, 0, S);
    constexpr int32_t kStep = LM_SUB / S;                               // between neighbouring samples
    uint32_t best[S * S];
#pragma unroll
    for (int s = 0; s < S * S; s++) best[s] = 0xffffffffu;
    const uint32_t begin = a.offsets[tile], end = min(a.offsets[tile + 1], a.pairs);
    for (uint32_t at = begin; at < end; at += 64u) {
        const uint32_t m = min(64u, end - at);
        __syncthreads();                                                // (the batch before has been read)
        if ((uint32_t)lane < m) {
            const uint32_t k = a.list[at + lane];
            lm_tri t; t.flags = 0u;
            if (k < (uint32_t)a.count) t = a.tris[k];
            lm_stage(t, (t.flags & LM_TRI_VALID) ? k : 0xffffffffu, staged[lane]);
        }
        __syncthreads();
        if (live) {
            for (uint32_t k = 0; k < m; k++) {
                const LmStaged &q = staged[k];
                int64_t e[3], sx[3], sy[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    e[c] = (int64_t)q.dx[c] * (int64_t)py0 - (int64_t)q.dy[c] * (int64_t)px0 + q.c[c];
                    sx[c] = -(int64_t)q.dy[c] * kStep; sy[c] = (int64_t)q.dx[c] * kStep;      // a step in i, a step in j
                }
#pragma unroll
                for (int j = 0; j < S; j++) {
#pragma unroll
                    for (int i = 0; i < S; i++) {
                        const int64_t e0 = e[0] + sx[0] * i + sy[0] * j, e1 = e[1] + sx[1] * i + sy[1] * j, e2 = e[2] + sx[2] * i + sy[2] * j;
                        if ((e0 | e1 | e2) >= 0) best[j * S + i] = min(best[j * S + i], q.index);
                    }
                }
            }
        }
    }
    if (!live) return;
    float4 *o = reinterpret_cast<float4 *>(a.out) + ((size_t)yl * (size_t)a.width + (size_t)x) * (size_t)(S * S);
#pragma unroll
    for (int j = 0; j < S; j++) {
#pragma unroll
        for (int i = 0; i < S; i++) {
            const uint32_t k = best[j * S + i];
            float4 h = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
            if (k != 0xffffffffu) {
                const lm_tri t = a.tris[k];
                float b = 0.f, g = 0.f;
                if (lm_cover(&t, px0 + kStep * i, py0 + kStep * j, &b, &g)) h = make_float4(0.f, b, g, __int_as_float(a.first + (int32_t)k));
            }
            o[j * S + i] = h;
        }
    }
}

__global__ __launch_bounds__(256) void lightmap_resolve_kernel(ResolveArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint32_t)a.texels) return;
    float4 vpl = make_float4(0.f, 0.f, 0.f, 0.f), pm = vpl;
    int32_t n = 0;
    for (int32_t s = 0; s < a.s2; s++) {                                // ascending (j, i): the samples' order in memory
        const size_t at = (size_t)i * (size_t)a.s2 + (size_t)s;
        if (a.points[4 * at].w != 1.0f) continue;
        const float4 l0 = a.lights[2 * at], l1 = a.lights[2 * at + 1];
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

__global__ __launch_bounds__(256) void lightmap_gutter_kernel(GutterArgs a) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)a.width * (size_t)a.height) return;
    const float4 *from = reinterpret_cast<const float4 *>(a.from);
    float4 t0 = from[2 * i], t1 = from[2 * i + 1];
    if (t0.w == 0.0f) {
        const int32_t x = (int32_t)(i % (size_t)a.width), y = (int32_t)(i / (size_t)a.width);
        float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
        int32_t n = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) {                                   // (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1)
            if (k == 4) continue;
            const int32_t nx = x + k % 3 - 1, ny = y + k / 3 - 1;
            if (nx < 0 || nx >= a.width || ny < 0 || ny >= a.height) continue;
            const size_t at = (size_t)ny * (size_t)a.width + (size_t)nx;
            const float4 n0 = from[2 * at];
            if (n0.w == 0.0f) continue;
            const float4 n1 = from[2 * at + 1];
            s0.x += n0.x; s0.y += n0.y; s0.z += n0.z; s1.x += n1.x; s1.y += n1.y; s1.z += n1.z; s1.w += n1.w;
            n++;
        }
        if (n > 0) {
            const float d = (float)n;
            t0 = make_float4(s0.x / d, s0.y / d, s0.z / d, -(float)a.pass);
            t1 = make_float4(s1.x / d, s1.y / d, s1.z / d, s1.w / d);
        }
    }
    float4 *to = reinterpret_cast<float4 *>(a.to);
    to[2 * i] = t0; to[2 * i + 1] = t1;
}

void launch_lightmap_points(const PointsArgs &a, hipStream_t s) {
    if (a.n <= 0) return;
    hipLaunchKernelGGL(lightmap_points_kernel, dim3((uint32_t)(((int64_t)a.n + 255) / 256)), dim3(256), 0, s, a);
}
void launch_lightmap_setup(const RasterArgs &a, hipStream_t s) {
    if (a.count <= 0) return;
    hipLaunchKernelGGL(lightmap_setup_kernel, dim3((uint32_t)(((int64_t)a.count + 255) / 256)), dim3(256), 0, s, a);
}
size_t lightmap_scan_temp_bytes(int32_t tiles) {
    size_t need = 0;
    uint32_t *none = nullptr;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, need, none, none, tiles + 1, (hipStream_t) nullptr) != hipSuccess) return 0;
    return need ? need : 1;
}
hipError_t launch_lightmap_count(const RasterArgs &a, void *temp, size_t temp_bytes, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.counts, 0, sizeof(uint32_t) * ((size_t)a.tiles + 1), s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(a.cursors, 0, sizeof(uint32_t) * (size_t)a.tiles, s);
    if (e != hipSuccess) return e;
    if (a.count > 0) hipLaunchKernelGGL(lightmap_count_kernel, dim3((uint32_t)(((int64_t)a.count + 255) / 256)), dim3(256), 0, s, a);
    size_t bytes = temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(temp, bytes, a.counts, a.offsets, a.tiles + 1, s);
}
void launch_lightmap_fill_raster(const RasterArgs &a, hipStream_t s) {
    if (a.count > 0 && a.pairs > 0u) hipLaunchKernelGGL(lightmap_fill_kernel, dim3((uint32_t)(((int64_t)a.count + 255) / 256)), dim3(256), 0, s, a);
    const dim3 grid((uint32_t)a.tiles), block(64);
    if (a.samples == 1) hipLaunchKernelGGL(lightmap_raster_kernel<1>, grid, block, 0, s, a);
    else if (a.samples == 2) hipLaunchKernelGGL(lightmap_raster_kernel<2>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(lightmap_raster_kernel<4>, grid, block, 0, s, a);
}
void launch_lightmap_resolve(const ResolveArgs &a, hipStream_t s) {
    if (a.texels <= 0) return;
    hipLaunchKernelGGL(lightmap_resolve_kernel, dim3((uint32_t)(((int64_t)a.texels + 255) / 256)), dim3(256), 0, s, a);
}
void launch_lightmap_gutter(const GutterArgs &a, hipStream_t s) {
    const size_t n = (size_t)a.width * (size_t)a.height;
    hipLaunchKernelGGL(lightmap_gutter_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, a);
}

} // namespace evplp
