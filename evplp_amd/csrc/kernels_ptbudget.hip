// Budget mode of the path tracer (evplp_adaptive_enable_pt(ctx, 2)): every tile takes its own number of samples of a batched call
// (kernels.h PtBudgetChunk explains the item table and the raw sums).
//   pt_budget_scan_kernel        first[t] = the exclusive prefix sum of the tiles' sample counts, one workgroup, no atomics
//   pt_budget_fill_kernel        table[first[t] + s] = t * 64 + s
//   pt_budget_trace_kernel       <- pt_batch_trace_kernel, (tile, sample) read from the table
//   pt_budget_accumulate_kernel  R += the chunk's staged samples of the tile, one at a time in increasing s
//   pt_budget_finish_kernel      n_t += s_t; VPL_ACCUM = (float)(R * (N / n_t))
// The batched primary of this mode lives in kernels_ptbudget_exact.hip (-ffp-contract=off); this unit keeps the path tracer's flags.
#include "device_common.hpp"
#include "pt_common.hpp"

namespace evplp {

// One workgroup walks the records in increasing tile index, 1024 at a time: an inclusive shuffle scan per wavefront, the wavefronts' totals
// added in wave order (pt_batch_list_kernel's shape with counts in place of ballot bits).  first [ntiles + 1]; first[ntiles] = the total.
__global__ __launch_bounds__(1024) void pt_budget_scan_kernel(const int4 *tiles, int32_t ntiles, int32_t samples, int32_t *first) {
    __shared__ uint32_t wave_counts[16];
    __shared__ uint32_t base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int32_t start = 0; start < ntiles; start += 1024) {
        const int32_t i = start + tid;
        uint32_t st = 0;
        if (i < ntiles) { const int32_t b = tiles[i].w; st = (uint32_t)(b < 0 ? samples : min(b, samples)); }
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
__global__ __launch_bounds__(64) void pt_budget_fill_kernel(const int32_t *first, uint32_t *table) {
    const int tile = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int f0 = __builtin_amdgcn_readfirstlane(first[tile]), f1 = __builtin_amdgcn_readfirstlane(first[tile + 1]);
    if (lane < f1 - f0) table[f0 + lane] = (uint32_t)tile * 64u + (uint32_t)lane;
}

#ifndef EVPLP_PT_WAVES
#define EVPLP_PT_WAVES 4   // as path_trace_kernel: 128 VGPRs, zero scratch
#endif
// slot = blockIdx.x, item = ch.item_first + slot.  The text is pt_batch_trace_kernel's but for where (tile, s) come from: the table entry,
// and with it the seed, are read ahead of every branch and through readfirstlane, so that the optimiser lists the operands of the first
// vertex's sampled direction as path_trace_kernel does (tests/test_pt_budget_resources.py holds the operand shapes).  The launch never
// exceeds the table (the host sizes both from the same budgets); the total's test still ends a surplus item.
__global__ __launch_bounds__(64, EVPLP_PT_WAVES) void pt_budget_trace_kernel(PathTraceArgs a, PtBatchSamples sm, PtBudgetChunk ch) {
    extern __shared__ int32_t lds_stack[];   // [bvh_depth + 2][64 lanes]
    const int lane = threadIdx.x;
    const int slot_i = (int)blockIdx.x, item = ch.item_first + slot_i;
    const uint32_t packed = __builtin_amdgcn_readfirstlane(ch.table[item]);
    const int s = (int)(packed & 63u);
    const uint32_t seed = __builtin_amdgcn_readfirstlane(sm.seed[s]);
    if (item >= *ch.total) return;
    const int tile = (int)(packed >> 6);
    const int tiles_x = (a.st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    const int y = a.st.global_row(min(ly, a.st.local_rows - 1));
    const bool in_image = x < a.st.W && ly < a.st.local_rows && y < a.st.H;
    PathTraceArgs v = a;
    v.g_pos = ch.staging; v.g_nrm = ch.staging + 64; v.g_dif = ch.staging + 128; v.g_phg = ch.staging + 192; v.out = ch.staging;
    v.rng_seed = seed;
    const size_t p = (size_t)slot_i * 256 + lane;
    const float4 gp = v.g_pos[p];
    const bool valid = in_image && gp.w != 0.0f;
    unsigned long long rays = 0, paths = valid ? 1ull : 0ull;
    if (valid) rays = path_trace_pixel(v, x, y, p, gp, lds_stack + lane);
    if (valid) reinterpret_cast<float *>(ch.staging + p)[3] = 1.0f;
    else ch.staging[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int off = 32; off > 0; off >>= 1) { rays += __shfl_xor(rays, off); paths += __shfl_xor(paths, off); }
    if (lane == 0 && a.counters && paths) { atomicAdd(&a.counters->rays, rays); atomicAdd(&a.counters->pairs, paths); }
}

// one wavefront per tile of the planes, lane = pixel: the items [first[t], first[t + 1]) that fall into the chunk, in increasing s, every add
// rounded to fp32 on its own (pt_batch_reduce_kernel's rule, applied to R)
__global__ __launch_bounds__(64) void pt_budget_accumulate_kernel(StripDev st, float4 *snap, const int32_t *first, PtBudgetChunk ch) {
    const int lane = threadIdx.x, tile = (int)blockIdx.x;
    const int f0 = __builtin_amdgcn_readfirstlane(first[tile]), f1 = __builtin_amdgcn_readfirstlane(first[tile + 1]);
    const int lo = max(f0, ch.item_first), hi = min(f1, ch.item_first + ch.item_count);
    if (lo >= hi) return;
    const int tiles_x = (st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    if (x >= st.W || ly >= st.local_rows || st.global_row(ly) >= st.H) return;
    const size_t p = (size_t)ly * st.W + x;
    const float4 *slot = ch.staging + (size_t)(lo - ch.item_first) * 256 + lane;
    float4 acc = snap[p];
    for (int k = 0; k < hi - lo; k++) {
        const float4 r = slot[(size_t)k * 256];
        if (r.w != 0.0f) { acc.x = __fadd_rn(acc.x, r.x); acc.y = __fadd_rn(acc.y, r.y); acc.z = __fadd_rn(acc.z, r.z); }
    }
    snap[p] = acc;
}

// one wavefront per tile of the planes, once per call after the last chunk; lane 0 writes the record after reading it wave-uniformly
__global__ __launch_bounds__(64) void pt_budget_finish_kernel(StripDev st, int4 *tiles, const int32_t *first, const float4 *snap, float4 *out, int32_t n_after) {
    const int lane = threadIdx.x, tile = (int)blockIdx.x;
    const int st_n = __builtin_amdgcn_readfirstlane(first[tile + 1]) - __builtin_amdgcn_readfirstlane(first[tile]);
    const int nt = __builtin_amdgcn_readfirstlane(tiles[tile].x) + st_n;
    if (lane == 0 && st_n != 0) reinterpret_cast<int32_t *>(tiles + tile)[0] = nt;
    if (nt == 0) return;
    const int tiles_x = (st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
    if (x >= st.W || ly >= st.local_rows || st.global_row(ly) >= st.H) return;
    const size_t p = (size_t)ly * st.W + x;
    const float4 R = snap[p];
    const double f = __ddiv_rn((double)n_after, (double)nt);
    out[p] = make_float4(__double2float_rn(__dmul_rn((double)R.x, f)), __double2float_rn(__dmul_rn((double)R.y, f)),
                         __double2float_rn(__dmul_rn((double)R.z, f)), __double2float_rn(__dmul_rn((double)R.w, f)));
}

void launch_pt_budget_table(const int4 *tiles, int32_t ntiles, int32_t samples, int32_t *first, uint32_t *table, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(pt_budget_scan_kernel, dim3(1), dim3(1024), 0, s, tiles, ntiles, samples, first);
    hipLaunchKernelGGL(pt_budget_fill_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, (const int32_t *)first, table);
}
void launch_pt_budget_trace(const PathTraceArgs &a, const PtBatchSamples &sm, const PtBudgetChunk &ch, hipStream_t s) {
    if (ch.item_count <= 0) return;
    const size_t lds = EVPLP_PT_WIDE ? lane_stack_bytes4(a.sc) : lane_stack_bytes(a.sc);
    hipLaunchKernelGGL(pt_budget_trace_kernel, dim3((unsigned)ch.item_count), dim3(64), lds, s, a, sm, ch);
}
void launch_pt_budget_accumulate(const StripDev &st, float4 *snap, const int32_t *first, int32_t ntiles, const PtBudgetChunk &ch, hipStream_t s) {
    if (ntiles <= 0 || ch.item_count <= 0) return;
    hipLaunchKernelGGL(pt_budget_accumulate_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, st, snap, first, ch);
}
void launch_pt_budget_finish(const StripDev &st, int4 *tiles, const int32_t *first, const float4 *snap, float4 *out, int32_t n_after, int32_t ntiles, hipStream_t s) {
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(pt_budget_finish_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, st, tiles, first, snap, out, n_after);
}

} // namespace evplp
