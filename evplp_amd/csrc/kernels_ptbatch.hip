// evplp_path_trace_batch: every tile takes its own number of the call's S samples, in every mode (kernels.h PtBatchChunk explains the item
// table, the staging slots and pt_tile_samples).
//   pt_batch_scan_kernel        first[t] = the exclusive prefix sum of the tiles' sample counts, one workgroup, no atomics
//   pt_batch_fill_kernel        table[first[t] + s] = t * 64 + s
//   pt_batch_trace_kernel       <- path_trace_kernel (kernels_pt.hip): one camera path per lane from the staged texels, result to the slot
//   pt_batch_accumulate_kernel  plane += the chunk's staged samples of the tile, one at a time in increasing s
//   pt_batch_close_kernel       modes 1 and 2, once per call: the pixels that are an extrapolation of the snapshot R
// The batched primary lives in kernels_ptbatch_primary.hip: it needs -ffp-contract=off for the whole translation unit, this one must not
// have it (a sample's radiance is path_trace_kernel's, compiled with contraction).
#include "device_common.hpp"
#include "pt_common.hpp"

namespace evplp {

// One workgroup walks the tiles in increasing index, 1024 at a time: an inclusive shuffle scan per wavefront, the wavefronts' totals added in
// wave order -- a prefix sum without atomics, so the table is the same on every run (compact_vpl_kernel's shape with counts in place of
// ballot bits).  tiles: the records, read in modes 1 and 2 only.  first [ntiles + 1]; first[ntiles] = the total.
__global__ __launch_bounds__(1024) void pt_batch_scan_kernel(const int4 *tiles, int32_t ntiles, int32_t mode, int32_t samples, int32_t *first) {
    __shared__ uint32_t wave_counts[16];
    __shared__ uint32_t base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int32_t start = 0; start < ntiles; start += 1024) {
        const int32_t i = start + tid;
        uint32_t st = 0;
        if (i < ntiles) st = (uint32_t)pt_tile_samples(mode, mode ? tiles[i] : make_int4(0, 0, 0, 0), samples);
        uint32_t incl = st;
        for (int off = 1; off < 64; off <<= 1) { const uint32_t up = __shfl_up(incl, off, 64); if (lane >= off) incl += up; }
        if (lane == 63) wave_counts[wave] = incl;
        __syncthreads();
        uint32_t off = base;
        for (int w = 0; w < wave; w++) off += wave_counts[w];
        if (i < ntiles) first[i] = (int32_t)(off + incl - st);
        __syncthreads();
        if (tid == 0) { uint32_t tot = 0; for (int w = 0; w < 16; w++) tot += wave_counts[w]; base += tot; }
        __syncthreads();
    }
    if (tid == 0) first[ntiles] = (int32_t)base;
}
// one wavefront per tile, lane = sample
__global__ __launch_bounds__(64) void pt_batch_fill_kernel(const int32_t *first, uint32_t *table) {
    const int tile = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int f0 = __builtin_amdgcn_readfirstlane(first[tile]), f1 = __builtin_amdgcn_readfirstlane(first[tile + 1]);
    if (lane < f1 - f0) table[f0 + lane] = (uint32_t)tile * 64u + (uint32_t)lane;
}

#ifndef EVPLP_PT_WAVES
#define EVPLP_PT_WAVES 4   // as path_trace_kernel: 128 VGPRs, zero scratch
#endif
// slot = blockIdx.x, item = ch.item_first + slot.  The stencil and the generator are path_trace_kernel's: a lane traces if its pixel is in the
// image and the staged position's w is not 0, keyed by (pixel, the sample's seed).  The lane calls path_trace_pixel itself -- the one text, see
// pt_common.hpp -- with a view of the arguments whose texel planes and `out` are the staging planes, indexed by the lane's slot word, and
// a.do_accumulate is 0 (the host sets it): plane 0 becomes 0 + radiance, and its w is then set to 1.  A lane that did not trace stores zeros
// (the accumulation adds nothing for it, as a single call leaves such a pixel alone).  Rays and paths: one atomic per wave, as there.
// The table entry, and with it the seed, are read HERE, ahead of every branch, and through readfirstlane, which the optimiser may not sink to
// its use.  Where the seed enters decides the order in which the optimiser lists the operands of n * p.z + (t * p.x + b * p.y) in the first
// vertex's lambert_sample, and the back end fuses the product it finds first: with the load beside the texel loads the other product was
// rounded, one unit in the last place off path_trace_kernel in a few pixels per frame (tests/test_pt_batch_same_arithmetic.py).  The launch
// never exceeds the table (the host sizes both with pt_tile_samples from the same records); the total's test still ends a surplus item.
__global__ __launch_bounds__(64, EVPLP_PT_WAVES) void pt_batch_trace_kernel(PathTraceArgs a, PtBatchSamples sm, PtBatchChunk ch) {
    extern __shared__ int32_t lds_stack[];   // [bvh_depth + 2][64 lanes]
    const int lane = threadIdx.x;
    const int slot_i = (int)blockIdx.x, item = ch.item_first + slot_i;
    // (a volatile read: a vector load.  As a scalar load the entry, which only 16 consecutive wavefronts share a cache line of, misses the
    // scalar cache at every 16th wavefront's start, and the misses hold up the scalar loads of the paths in flight around it: 0.6 % of the
    // kernel at 1024^2, profiles/pt_batch_table.txt)
    const uint32_t packed = __builtin_amdgcn_readfirstlane(*(const volatile uint32_t *)(ch.table + item));
    const int s = (int)(packed & 63u);
    const uint32_t seed = __builtin_amdgcn_readfirstlane(sm.seed[s]);
    if (item >= *ch.total) return;
    const int2 xl = tile_lane((int)(packed >> 6), lane, a.st.W);
    const int x = xl.x, ly = xl.y;
    const int y = a.st.global_row(min(ly, a.st.local_rows - 1));
    const bool in_image = x < a.st.W && ly < a.st.local_rows && y < a.st.H;
    // the view: wave-uniform plane pointers and a per-lane index, the addressing path_trace_kernel has
    PathTraceArgs v = a;
    v.g_pos = ch.staging; v.g_nrm = ch.staging + 64; v.g_dif = ch.staging + 128; v.g_phg = ch.staging + 192; v.out = ch.staging;
    v.rng_seed = seed;
    const size_t p = (size_t)slot_i * 256 + lane;
    const float4 gp = v.g_pos[p];
    const bool valid = in_image && gp.w != 0.0f;                          // stencil (:357)
    unsigned long long rays = 0, paths = valid ? 1ull : 0ull;
    if (valid) rays = path_trace_pixel(v, x, y, p, gp, lds_stack + lane);
    if (valid) reinterpret_cast<float *>(ch.staging + p)[3] = 1.0f;
    else ch.staging[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int off = 32; off > 0; off >>= 1) { rays += __shfl_xor(rays, off); paths += __shfl_xor(paths, off); }
    if (lane == 0 && a.counters && paths) { atomicAdd(&a.counters->rays, rays); atomicAdd(&a.counters->pairs, paths); }
}

// one wavefront per tile of the planes, lane = pixel: acc = plane; acc += r_s for the items of [first[t], first[t + 1]) that fall into the
// chunk, in increasing s, every add rounded to fp32 on its own (out + r0 + r1, never out + (r0 + r1)); one store.  w is carried, as
// path_trace_kernel carries it.  plane: VPL_ACCUM, or the snapshot R in budget mode.
__global__ __launch_bounds__(64) void pt_batch_accumulate_kernel(StripDev st, float4 *plane, const int32_t *first, PtBatchChunk ch) {
    const int lane = threadIdx.x, tile = (int)blockIdx.x;
    const int f0 = __builtin_amdgcn_readfirstlane(first[tile]), f1 = __builtin_amdgcn_readfirstlane(first[tile + 1]);
    const int lo = max(f0, ch.item_first), hi = min(f1, ch.item_first + ch.item_count);
    if (lo >= hi) return;
    const int2 xl = tile_lane(tile, lane, st.W);
    const int x = xl.x, ly = xl.y;
    if (x >= st.W || ly >= st.local_rows || st.global_row(ly) >= st.H) return;
    const size_t p = (size_t)ly * st.W + x;
    const float4 *slot = ch.staging + (size_t)(lo - ch.item_first) * 256 + lane;
    float4 acc = plane[p];
    for (int k = 0; k < hi - lo; k++) {
        const float4 r = slot[(size_t)k * 256];
        if (r.w != 0.0f) { acc.x = __fadd_rn(acc.x, r.x); acc.y = __fadd_rn(acc.y, r.y); acc.z = __fadd_rn(acc.z, r.z); }
    }
    plane[p] = acc;
}

// one wavefront per tile of the planes, once per call after the last chunk: out = (float)(R * (n_after / n_t)) for a tile with n_t != 0
// (path_trace_kernel<true>'s arithmetic, once for the S samples).  Mode 1: n_t is the record's, so the retired tiles are written and an
// active tile's wavefront exits at once.  Mode 2: n_t += s_t first; lane 0 writes the record after the wavefront has read it uniformly.
__global__ __launch_bounds__(64) void pt_batch_close_kernel(StripDev st, int4 *tiles, int32_t mode, const int32_t *first, const float4 *snap, float4 *out, int32_t n_after) {
    const int lane = threadIdx.x, tile = (int)blockIdx.x;
    int nt = __builtin_amdgcn_readfirstlane(tiles[tile].x);
    if (mode == 2) {
        const int st_n = __builtin_amdgcn_readfirstlane(first[tile + 1]) - __builtin_amdgcn_readfirstlane(first[tile]);
        nt += st_n;
        if (lane == 0 && st_n != 0) reinterpret_cast<int32_t *>(tiles + tile)[0] = nt;
    }
    if (nt == 0) return;
    const int2 xl = tile_lane(tile, lane, st.W);
    const int x = xl.x, ly = xl.y;
    if (x >= st.W || ly >= st.local_rows || st.global_row(ly) >= st.H) return;
    const size_t p = (size_t)ly * st.W + x;
    out[p] = extrapolate(snap[p], n_after, nt);
}

void launch_pt_batch_table(const int4 *tiles, int32_t ntiles, int32_t mode, int32_t samples, int32_t *first, uint32_t *table, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(pt_batch_scan_kernel, dim3(1), dim3(1024), 0, s, tiles, ntiles, mode, samples, first);
    hipLaunchKernelGGL(pt_batch_fill_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, (const int32_t *)first, table);
}
void launch_pt_batch_trace(const PathTraceArgs &a, const PtBatchSamples &sm, const PtBatchChunk &ch, hipStream_t s) {
    if (ch.item_count <= 0) return;
    const size_t lds = EVPLP_PT_WIDE ? lane_stack_bytes4(a.sc) : lane_stack_bytes(a.sc);
    hipLaunchKernelGGL(pt_batch_trace_kernel, dim3((unsigned)ch.item_count), dim3(64), lds, s, a, sm, ch);
}
void launch_pt_batch_accumulate(const StripDev &st, float4 *plane, const int32_t *first, int32_t ntiles, const PtBatchChunk &ch, hipStream_t s) {
    if (ntiles <= 0 || ch.item_count <= 0) return;
    hipLaunchKernelGGL(pt_batch_accumulate_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, st, plane, first, ch);
}
void launch_pt_batch_close(const StripDev &st, int4 *tiles, int32_t mode, const int32_t *first, const float4 *snap, float4 *out, int32_t n_after, int32_t ntiles, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(pt_batch_close_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, st, tiles, mode, first, snap, out, n_after);
}

} // namespace evplp
