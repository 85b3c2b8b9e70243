// Unidirectional path tracer with next-event estimation: the reference's own ground-truth technique
// ("pt" block of the scene JSON, rt/rtpt/rtpt2.h) and the generator of converged images for the
// convergence tests.
//   path_trace_kernel  <- splatColor + pathTraceSimple (rt/pathtracing.cu:350-377, 240-348) with the
//                         closest-hit program inlined as the bounce loop (rt/pathtracing.cu:112-228)
// One lane per pixel of an 8x8 tile; after the first bounce the rays of a wave are incoherent, so both the
// closest-hit and the shadow walk are per-lane with the [entry][lane] LDS stack of the feeder kernels.
#include "device_common.hpp"
#include "pt_common.hpp"

namespace evplp {

#ifndef EVPLP_PT_WAVES
#define EVPLP_PT_WAVES 4   // 128 VGPRs, zero scratch (126 needed): 1.61 ms per sample per pixel at 1024^2 against 1.59 ms at 6 waves with 65 spilled registers
#endif
// ADAPT (evplp_adaptive_enable_pt): one wave-uniform scalar read of the tile's record (kernels.h AdaptTiles; .x = n_t, 0: active) right after
// the tile index is known.  A retired tile reads neither the G-buffer nor the LDS stack, traces nothing and adds nothing to the counters: its
// pixels inside the strip -- whatever the stencil says -- become the snapshot R extrapolated to N + 1 iterations, in gather_reduce_kernel<true>'s
// arithmetic: (float)(R * ((N + 1) / n_t)) per channel in fp64.  An active tile runs as in the default; ad is read by this variant only.
template <bool ADAPT = false>
__global__ __launch_bounds__(64, EVPLP_PT_WAVES) void path_trace_kernel(PathTraceArgs a, AdaptArgs ad) {
    extern __shared__ int32_t lds_stack[];   // [bvh_depth + 2][64 lanes]
    const int lane = threadIdx.x;
    const int tile = blockIdx.x;
    const int2 xl = tile_lane(tile, lane, a.st.W);
    const int x = xl.x, ly = xl.y;
    const int y = a.st.global_row(min(ly, a.st.local_rows - 1));
    const bool in_image = x < a.st.W && ly < a.st.local_rows && y < a.st.H;
    const size_t p = (size_t)min(ly, a.st.local_rows - 1) * a.st.W + min(x, a.st.W - 1);
    if constexpr (ADAPT) {
        const int nt = __builtin_amdgcn_readfirstlane(ad.tiles[tile].x);
        if (nt != 0) {
            if (in_image) a.out[p] = extrapolate(ad.snap[p], ad.n1, nt);
            return;
        }
    }
    const float4 gp = a.g_pos[p];
    const bool valid = in_image && gp.w != 0.0f;                          // stencil (:357)
    unsigned long long rays = 0, paths = valid ? 1ull : 0ull;
    if (valid) rays = path_trace_pixel(a, x, y, p, gp, lds_stack + lane);
    // statistics: one atomic per wave
    for (int off = 32; off > 0; off >>= 1) { rays += __shfl_xor(rays, off); paths += __shfl_xor(paths, off); }
    if (lane == 0 && a.counters && paths) { atomicAdd(&a.counters->rays, rays); atomicAdd(&a.counters->pairs, paths); }
}

// ad.tiles set: the ADAPT variant (evplp_path_trace in path-trace mode); the same tile grid either way
void launch_path_trace(const PathTraceArgs &a, hipStream_t s, const AdaptArgs &ad) {
    int tiles_x = (a.st.W + 7) / 8, tiles_y = (a.st.local_rows + 7) / 8;
    if (tiles_x * tiles_y == 0) return;
    const size_t lds = EVPLP_PT_WIDE ? lane_stack_bytes4(a.sc) : lane_stack_bytes(a.sc);
    if (ad.tiles) hipLaunchKernelGGL(path_trace_kernel<true>, dim3(tiles_x * tiles_y), dim3(64), lds, s, a, ad);
    else hipLaunchKernelGGL(path_trace_kernel<false>, dim3(tiles_x * tiles_y), dim3(64), lds, s, a, ad);
}

} // namespace evplp
