// evplp_path_trace_batch: S samples of the ACTIVE tiles in one call (kernels.h PtBatchChunk explains the items and the staging slots).
//   pt_batch_list_kernel     the active tiles, compacted in increasing order (adaptive mode; otherwise the list is the identity)
//   pt_batch_trace_kernel    <- path_trace_kernel (kernels_pt.hip): one camera path per lane from the staged texels, result to the slot
//   pt_batch_reduce_kernel   VPL_ACCUM += the staged samples, one at a time in increasing s
//   pt_batch_rescale_kernel  the retired tiles' pixels from the snapshot (path_trace_kernel<true>'s arithmetic, once for the S samples)
// The batched primary lives in kernels_ptbatch_primary.hip: it needs -ffp-contract=off for the whole translation unit, this one must not
// have it (a sample's radiance is path_trace_kernel's, compiled with contraction).
#include "device_common.hpp"
#include "pt_common.hpp"

namespace evplp {

// One workgroup scans the tile records in order: a ballot per wavefront, the wavefronts' counts added in wave order -- a prefix sum
// without atomics, so the list is the same on every run (compact_vpl_kernel's shape).  list [ntiles], count [1].
__global__ __launch_bounds__(1024) void pt_batch_list_kernel(const int4 *tiles, int32_t ntiles, int32_t *list, int32_t *count) {
    __shared__ uint32_t wave_counts[16];
    __shared__ uint32_t base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int32_t start = 0; start < ntiles; start += 1024) {
        const int32_t i = start + tid;
        const bool active = i < ntiles && tiles[i].x == 0;
        const unsigned long long m = __ballot(active);
        const uint32_t prefix = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_counts[wave] = __popcll(m);
        __syncthreads();
        uint32_t off = base;
        for (int w = 0; w < wave; w++) off += wave_counts[w];
        if (active) list[off + prefix] = i;
        __syncthreads();
        if (tid == 0) { uint32_t tot = 0; for (int w = 0; w < 16; w++) tot += wave_counts[w]; base += tot; }
        __syncthreads();
    }
    if (tid == 0) *count = (int32_t)base;
}

#ifndef EVPLP_PT_WAVES
#define EVPLP_PT_WAVES 4   // as path_trace_kernel: 128 VGPRs, zero scratch
#endif
// item = blockIdx.x.  The stencil and the generator are path_trace_kernel's: a lane traces if its pixel is in the image and the staged
// position's w is not 0, keyed by (pixel, the sample's seed).  The lane calls path_trace_pixel itself -- the one text, see pt_common.hpp --
// with a view of the arguments whose texel planes and `out` are the staging planes, indexed by the lane's slot word, and a.do_accumulate is 0
// (the host sets it): plane 0 becomes 0 + radiance, and its w is then set to 1.  A lane that did not trace stores zeros (the reduce adds
// nothing for it, as a single call leaves such a pixel alone).  Rays and paths: one atomic per wave, as there.
__global__ __launch_bounds__(64, EVPLP_PT_WAVES) void pt_batch_trace_kernel(PathTraceArgs a, PtBatchSamples sm, PtBatchChunk ch) {
    extern __shared__ int32_t lds_stack[];   // [bvh_depth + 2][64 lanes]
    const int lane = threadIdx.x;
    const int item = (int)blockIdx.x;
    const int el = item / ch.sample_count, s = ch.sample_first + (item - el * ch.sample_count);
    // The seed is read HERE, ahead of every branch, and through readfirstlane, which the optimiser may not sink to its use.  Where the seed
    // enters decides the order in which the optimiser lists the operands of n * p.z + (t * p.x + b * p.y) in the first vertex's
    // lambert_sample, and the back end fuses the product it finds first: with the load beside the texel loads the other product was
    // rounded, one unit in the last place off path_trace_kernel in a few pixels per frame (tests/test_pt_batch_same_arithmetic.py).
    const uint32_t seed = __builtin_amdgcn_readfirstlane(sm.seed[s]);
    const int e = ch.entry_first + el;
    const int n = ch.count ? *ch.count : ch.tiles;
    if (e >= n) return;
    const int tile = ch.list ? ch.list[e] : e;
    const int tiles_x = (a.st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    const int y = a.st.global_row(min(ly, a.st.local_rows - 1));
    const bool in_image = x < a.st.W && ly < a.st.local_rows && y < a.st.H;
    // the view: wave-uniform plane pointers and a per-lane index, the addressing path_trace_kernel has
    PathTraceArgs v = a;
    v.g_pos = ch.staging; v.g_nrm = ch.staging + 64; v.g_dif = ch.staging + 128; v.g_phg = ch.staging + 192; v.out = ch.staging;
    v.rng_seed = seed;
    const size_t p = (size_t)item * 256 + lane;
    const float4 gp = v.g_pos[p];
    const bool valid = in_image && gp.w != 0.0f;                          // stencil (:357)
    unsigned long long rays = 0, paths = valid ? 1ull : 0ull;
    if (valid) rays = path_trace_pixel(v, x, y, p, gp, lds_stack + lane);
    if (valid) reinterpret_cast<float *>(ch.staging + p)[3] = 1.0f;
    else ch.staging[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int off = 32; off > 0; off >>= 1) { rays += __shfl_xor(rays, off); paths += __shfl_xor(paths, off); }
    if (lane == 0 && a.counters && paths) { atomicAdd(&a.counters->rays, rays); atomicAdd(&a.counters->pairs, paths); }
}

// one wavefront per list entry of the chunk, lane = pixel: acc = out; acc += r_s for the chunk's samples in increasing s, every add
// rounded to fp32 on its own (out + r0 + r1, never out + (r0 + r1)); one store.  w is carried, as path_trace_kernel carries it.
__global__ __launch_bounds__(64) void pt_batch_reduce_kernel(StripDev st, float4 *out, PtBatchChunk ch) {
    const int lane = threadIdx.x;
    const int el = (int)blockIdx.x, e = ch.entry_first + el;
    const int n = ch.count ? *ch.count : ch.tiles;
    if (e >= n) return;
    const int tile = ch.list ? ch.list[e] : e;
    const int tiles_x = (st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    if (x >= st.W || ly >= st.local_rows || st.global_row(ly) >= st.H) return;
    const size_t p = (size_t)ly * st.W + x;
    const float4 *slot = ch.staging + (size_t)el * ch.sample_count * 256 + lane;
    float4 acc = out[p];
    for (int k = 0; k < ch.sample_count; k++) {
        const float4 r = slot[(size_t)k * 256];
        if (r.w != 0.0f) { acc.x = __fadd_rn(acc.x, r.x); acc.y = __fadd_rn(acc.y, r.y); acc.z = __fadd_rn(acc.z, r.z); }
    }
    out[p] = acc;
}

// one wavefront per tile of the planes; an active tile's exits at once
__global__ __launch_bounds__(64) void pt_batch_rescale_kernel(StripDev st, float4 *out, AdaptArgs ad) {
    const int lane = threadIdx.x;
    const int tile = (int)blockIdx.x;
    const int nt = __builtin_amdgcn_readfirstlane(ad.tiles[tile].x);
    if (nt == 0) return;
    const int tiles_x = (st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    if (x >= st.W || ly >= st.local_rows || st.global_row(ly) >= st.H) return;
    const size_t p = (size_t)ly * st.W + x;
    const float4 R = ad.snap[p];
    const double f = __ddiv_rn((double)ad.n1, (double)nt);
    out[p] = make_float4(__double2float_rn(__dmul_rn((double)R.x, f)), __double2float_rn(__dmul_rn((double)R.y, f)),
                         __double2float_rn(__dmul_rn((double)R.z, f)), __double2float_rn(__dmul_rn((double)R.w, f)));
}

void launch_pt_batch_list(const int4 *tiles, int32_t ntiles, int32_t *list, int32_t *count, hipStream_t s) {
    hipLaunchKernelGGL(pt_batch_list_kernel, dim3(1), dim3(1024), 0, s, tiles, ntiles, list, count);
}
void launch_pt_batch_trace(const PathTraceArgs &a, const PtBatchSamples &sm, const PtBatchChunk &ch, hipStream_t s) {
    const long long items = (long long)ch.entry_count * ch.sample_count;
    if (items <= 0) return;
    const size_t lds = EVPLP_PT_WIDE ? lane_stack_bytes4(a.sc) : lane_stack_bytes(a.sc);
    hipLaunchKernelGGL(pt_batch_trace_kernel, dim3((unsigned)items), dim3(64), lds, s, a, sm, ch);
}
void launch_pt_batch_reduce(const StripDev &st, float4 *out, const PtBatchChunk &ch, hipStream_t s) {
    if (ch.entry_count <= 0 || ch.sample_count <= 0) return;
    hipLaunchKernelGGL(pt_batch_reduce_kernel, dim3((unsigned)ch.entry_count), dim3(64), 0, s, st, out, ch);
}
void launch_pt_batch_rescale(const StripDev &st, float4 *out, const AdaptArgs &ad, int32_t ntiles, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(pt_batch_rescale_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, st, out, ad);
}

} // namespace evplp
