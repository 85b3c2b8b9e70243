// Temporal accumulation in front of the a-trous passes (evplp_denoise_temporal, include/evplp.h): the temporal half of SVGF (Schied et al.
// 2017) by backward reprojection.
//   prev_pose_kernel            the primary walk again, one wavefront per 8 x 8 tile: every pixel's hit evaluated on the PREVIOUS pose
//   pose_snapshot_kernel        TriAttr::v -> the previous pose, 9 floats per original triangle, at the end of a call
//   temporal_accumulate_kernel  one thread per pixel of the frame the context filters: motion, the 2 x 2 taps of the history, the blend
// The unit is compiled without floating-point contraction (Makefile), as kernels_trace.hip and kernels_denoise.hip are: the hit (tri, b, g)
// must be the one of the G-buffer in memory and P, N on an unmoved pose must carry that G-buffer's bits; the accumulation stage uses
// + - * /, floor, min, max and compares only, each rounded on its own, and tests/temporal_restate.py follows it bit for bit.
#include "device_common.hpp"
#include "kernels.h"

namespace evplp {

// Launched like primary_kernel, with its arguments (launch_primary, kernels_trace.hip: the same deal of tiles to workgroups).  The walks are
// wave-collective: no early return before them, and lanes outside the image stay in the wave.  The material fetch of the shared body has no
// reader here and is dropped by the compiler.
__global__ __launch_bounds__(64) void prev_pose_kernel(PrimaryArgs a, const float *prev_v, TemporalPrev *prev, float4 *debug) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int tiles_x = (a.st.W + 7) >> 3;
#if EVPLP_PRIMARY_BLOCKS
    constexpr int L = EVPLP_PRIMARY_BLOCK_LOG2, B = 1 << L;
    const int tiles_y = (a.st.local_rows + 7) >> 3, nbx = (tiles_x + B - 1) >> L;
    const int bj = (int)blockIdx.x >> 3, blk = (bj >> (2 * L)) * 8 + ((int)blockIdx.x & 7), within = bj & (B * B - 1);
    const int tx = (blk % nbx) * B + (within & (B - 1)), ty = (blk / nbx) * B + (within >> L);
    if (tx >= tiles_x || ty >= tiles_y) return;                     // padding of the block grid (wave-uniform)
#else
    const int tx = (int)blockIdx.x % tiles_x, ty = (int)blockIdx.x / tiles_x;
#endif
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    const int y = a.st.global_row(min(ly, a.st.local_rows - 1));
    const bool in_image = x < a.st.W && ly < a.st.local_rows && y < a.st.H;   // no early return: the walk is wave-collective
    const size_t p = (size_t)min(ly, a.st.local_rows - 1) * a.st.W + min(x, a.st.W - 1);

#define PRIMARY_JIT0 a.jitter[0]
#define PRIMARY_JIT1 a.jitter[1]
#define PRIMARY_USE_CUT a.cuts
#include "primary_body.hpp"
#undef PRIMARY_JIT0
#undef PRIMARY_JIT1
#undef PRIMARY_USE_CUT
    if (!in_image) return;
    float4 pp = make_float4(0.f, 0.f, 0.f, 0.f), pn = pp;
    if (tri >= 0 && prev) {
        // the body's two expressions for P and N, on the previous vertices
        const float *pv = prev_v + 9 * (size_t)tri;
        V3 q0 = v3(pv), q1 = v3(pv + 3), q2 = v3(pv + 6);
        const float w0 = 1.0f - b - g;
        V3 P = v3((q1.x * b + q2.x * g) + q0.x * w0, (q1.y * b + q2.y * g) + q0.y * w0, (q1.z * b + q2.z * g) + q0.z * w0);
        V3 N = normalize_exact(cross_exact(q1 - q0, q2 - q0));
        pp = make_float4(P.x, P.y, P.z, 1.0f);
        pn = make_float4(N.x, N.y, N.z, 0.f);
    }
    if (prev) { prev[p].pos = pp; prev[p].nrm = pn; }
    if (debug) debug[p] = tri >= 0 ? make_float4(__int_as_float(tri), b, g, 0.f) : make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
}
void launch_prev_pose(const PrimaryArgs &a, const float *prev_v, TemporalPrev *prev, float4 *debug, hipStream_t s) {
    int tiles_x = (a.st.W + 7) / 8, tiles_y = (a.st.local_rows + 7) / 8;
#if EVPLP_PRIMARY_BLOCKS
    constexpr int B = 1 << EVPLP_PRIMARY_BLOCK_LOG2;
    const int blocks = ((tiles_x + B - 1) / B) * ((tiles_y + B - 1) / B);
    if (blocks == 0) return;
    hipLaunchKernelGGL(prev_pose_kernel, dim3((unsigned)((blocks + 7) / 8 * 8 * B * B)), dim3(64), 0, s, a, prev_v, prev, debug);
#else
    if (tiles_x * tiles_y == 0) return;
    hipLaunchKernelGGL(prev_pose_kernel, dim3(tiles_x * tiles_y), dim3(64), 0, s, a, prev_v, prev, debug);
#endif
}

// the reverse of refit_rest_kernel's strided copy (bvh_gpu.hip), over the whole scene
__global__ __launch_bounds__(256) void pose_snapshot_kernel(const TriAttr *attrs, int32_t ntri, float *prev_v) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 9 * (size_t)ntri) return;
    prev_v[i] = attrs[i / 9].v[i % 9];
}
void launch_pose_snapshot(const TriAttr *attrs, int32_t ntri, float *prev_v, hipStream_t s) {
    if (ntri > 0) hipLaunchKernelGGL(pose_snapshot_kernel, dim3((unsigned)((9 * (size_t)ntri + 255) / 256)), dim3(256), 0, s, attrs, ntri, prev_v);
}

// One thread per pixel, 16 x 16 pixels per workgroup as the a-trous passes.  Steps 1 - 5 of include/evplp.h evplp_denoise_temporal.  A thread
// reads its own packed pixel and previous-pose texel and up to four pixels of the OLD history, and writes its own pixel of the frame and of
// the NEW history: nothing it reads is written in this launch.  The four counts are integer sums, one slot per workgroup.
__global__ __launch_bounds__(256) void temporal_accumulate_kernel(TemporalArgs a) {
    const int x = (int)(blockIdx.x * 16 + (threadIdx.x & 15)), y = (int)(blockIdx.y * 16 + (threadIdx.x >> 4));
    unsigned filtered = 0, reprojected = 0, disoccluded = 0, length = 0;
    if (x < a.W && y < a.rows) {
        const size_t i = (size_t)y * a.W + x;
        const float4 u = a.frame[i].u, X = a.frame[i].pos, n = a.frame[i].nrm;
        float4 uo = u;
        float len = 0.0f;
        if (X.w != 0.0f) {
            filtered = 1; len = 1.0f;
            float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, ss = 0.0f, nmin = 3.0e38f;
            TemporalPrev pv; pv.pos = make_float4(0.f, 0.f, 0.f, 0.f); pv.nrm = pv.pos;
            if (a.has_history) pv = a.prev[i];
            if (pv.pos.w != 0.0f) {
                const float P[3] = { pv.pos.x, pv.pos.y, pv.pos.z }, N[3] = { pv.nrm.x, pv.nrm.y, pv.nrm.z }, Xc[3] = { X.x, X.y, X.z };
                float was[3], is[3];
                const bool seen = project_point(a.prev_cam, a.W, a.H, P, was), sees = project_point(a.cam, a.W, a.H, Xc, is);
                const float fx = (float)x + (was[0] - is[0]), fy = (float)y + (was[1] - is[1]);
                if (seen && sees && fx > -1.0f && fx < (float)a.W && fy > -1.0f && fy < (float)a.H) {
                    const float flx = floorf(fx), fly = floorf(fy), tx = fx - flx, ty = fy - fly;
                    const int ix = (int)flx, iy = (int)fly;
                    const bool integral = tx == 0.0f && ty == 0.0f;
                    // taps (0, 0), (1, 0), (0, 1), (1, 1) with the weights (k & 1 ? tx : 1 - tx) * (k >> 1 ? ty : 1 - ty); an integral position: the first alone, weight 1
                    for (int k = 0; k < 4; k++) {
                        if (integral && k > 0) break;
                        const int qx = ix + (k & 1), qy = iy + (k >> 1);
                        if (qx < 0 || qx >= a.W || qy < 0 || qy >= a.H) continue;
                        const size_t q = (size_t)qy * a.W + qx;
                        const float4 hx = a.h_in[a.px + q];
                        if (hx.w == 0.0f) continue;
                        const float4 hn = a.h_in[2 * a.px + q];
                        const float d1 = fabsf((hn.x * (P[0] - hx.x) + hn.y * (P[1] - hx.y)) + hn.z * (P[2] - hx.z));
                        const float d2 = fabsf((N[0] * (hx.x - P[0]) + N[1] * (hx.y - P[1])) + N[2] * (hx.z - P[2]));
                        const float cs = (N[0] * hn.x + N[1] * hn.y) + N[2] * hn.z;
                        if (!(d1 <= a.sigma_x_r) || !(d2 <= a.sigma_x_r) || !(cs >= a.normal_cos)) continue;
                        const float4 hu = a.h_in[q];
                        const float w = integral ? 1.0f : ((k & 1) ? tx : 1.0f - tx) * ((k >> 1) ? ty : 1.0f - ty);
                        sw = sw + w;
                        sr = sr + w * hu.x; sg = sg + w * hu.y; sb = sb + w * hu.z;
                        ss = ss + (w * w) * hu.w;
                        nmin = fminf(nmin, hn.w);
                    }
                }
            }
            if (sw > 0.0f) {
                reprojected = 1;
                len = fminf(nmin + 1.0f, a.max_history);
                const float al = 1.0f / len, be = 1.0f - al;
                const float hs = ss / (sw * sw);
                uo.x = be * (sr / sw) + al * u.x; uo.y = be * (sg / sw) + al * u.y; uo.z = be * (sb / sw) + al * u.z;
                uo.w = (be * be) * hs + (al * al) * u.w;
            } else if (a.has_history) disoccluded = 1;
            length = (unsigned)len;
            a.frame[i].u = uo;
        }
        a.h_out[i] = uo;
        a.h_out[a.px + i] = make_float4(X.x, X.y, X.z, X.w != 0.0f ? 1.0f : 0.0f);
        a.h_out[2 * a.px + i] = make_float4(n.x, n.y, n.z, len);
    }
    // the counts: over the wave by shuffles, over the workgroup's four waves through LDS, one slot per workgroup -- the host adds the slots
    // in their order (integers: any order gives the same sums; no atomics, which four hot addresses would serialise)
    for (int off = 32; off > 0; off >>= 1) {
        filtered += __shfl_xor(filtered, off); reprojected += __shfl_xor(reprojected, off);
        disoccluded += __shfl_xor(disoccluded, off); length += __shfl_xor(length, off);
    }
    __shared__ uint4 part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = make_uint4(filtered, reprojected, disoccluded, length);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint4 p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3];
        a.counts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = make_uint4(p0.x + p1.x + p2.x + p3.x, p0.y + p1.y + p2.y + p3.y, p0.z + p1.z + p2.z + p3.z, p0.w + p1.w + p2.w + p3.w);
    }
}
int temporal_count_slots(int W, int rows) { return ((W + 15) / 16) * ((rows + 15) / 16); }
void launch_temporal_accumulate(const TemporalArgs &a, hipStream_t s) {
    if (a.W <= 0 || a.rows <= 0) return;
    hipLaunchKernelGGL(temporal_accumulate_kernel, dim3((unsigned)((a.W + 15) / 16), (unsigned)((a.rows + 15) / 16)), dim3(256), 0, s, a);
}

} // namespace evplp
