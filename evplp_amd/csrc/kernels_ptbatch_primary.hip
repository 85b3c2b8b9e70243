// evplp_path_trace_batch (kernels.h PtBatchChunk), the kernels that must round every operation on its own: this unit is built like
// kernels_trace.hip, with -ffp-contract=off (Makefile).  The texels must carry the bits evplp_primary gives them, and those depend on inlined
// helpers that no pragma inside the kernel reaches (primary_body.hpp).  That is also why a chunk is two kernels in two translation units and
// not one fused kernel: the path tracer keeps contraction.
//   pt_batch_primary_kernel   <- primary_kernel (kernels_trace.hip), one wavefront per item of the table instead of per tile
//   noise_fold_budget_kernel  evplp_noise_fold per tile in budget mode, k_t = n_t - K_t
//   tile_noise_kernel         evplp_adaptive_tile_noise: adaptive_retire_kernel's per-tile mean, written out instead of compared
#include "device_common.hpp"
#include "kernels.h"
#include "noise_common.hpp"

namespace evplp {

// slot = blockIdx.x, item = ch.item_first + slot.  The packet walks start from the camera's entry cuts, which hold for every jitter up to a
// pixel (ch.cut_mask says which samples stay within that); the four texels of all 64 lanes go to the item's slot, nothing to the G-buffer
// planes.  The light plane gets the emitter colour where primary_kernel would put it under flags 0: every sample writes the same
// value, so concurrent items of one tile do not race.  a.clear_light is 0.
__global__ __launch_bounds__(64) void pt_batch_primary_kernel(PrimaryArgs a, PtBatchSamples sm, PtBatchChunk ch) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int slot_i = (int)blockIdx.x, item = ch.item_first + slot_i;
    if (item >= *ch.total) return;                                        // (wave-uniform: scalar loads)
    const uint32_t packed = __builtin_amdgcn_readfirstlane(*(const volatile uint32_t *)(ch.table + item));   // (a vector load, as in the trace)
    const int tile = (int)(packed >> 6), s = (int)(packed & 63u);
    const int2 txy = tile_coords(tile, a.st.W), xl = tile_lane(tile, lane, a.st.W);
    const int tx = txy.x, ty = txy.y, x = xl.x, ly = xl.y;                // (tx, ty: wave-uniform, the entry cuts' group)
    const int y = a.st.global_row(min(ly, a.st.local_rows - 1));
    const bool in_image = x < a.st.W && ly < a.st.local_rows && y < a.st.H;   // no early return: the walk is wave-collective
    const size_t p = (size_t)min(ly, a.st.local_rows - 1) * a.st.W + min(x, a.st.W - 1);
    const float jit0 = sm.jitter[s][0], jit1 = sm.jitter[s][1];
    const bool use_cut = a.cuts && ((ch.cut_mask >> s) & 1ull) != 0ull;

#define PRIMARY_JIT0 jit0
#define PRIMARY_JIT1 jit1
#define PRIMARY_USE_CUT use_cut
#include "primary_body.hpp"
#undef PRIMARY_JIT0
#undef PRIMARY_JIT1
#undef PRIMARY_USE_CUT

    float4 *slot = ch.staging + (size_t)slot_i * 256 + lane;              // [plane][lane]: every store of the wave is one contiguous KB
    slot[0] = pos; slot[64] = nrm; slot[128] = dif; slot[192] = phg;
    if (in_image && light_visible) a.g_light[p] = make_float4(a.sc.light_unscaled[0], a.sc.light_unscaled[1], a.sc.light_unscaled[2], 0.f);
}
void launch_pt_batch_primary(const PrimaryArgs &a, const PtBatchSamples &sm, const PtBatchChunk &ch, hipStream_t s) {
    if (ch.item_count <= 0) return;
    hipLaunchKernelGGL(pt_batch_primary_kernel, dim3((unsigned)ch.item_count), dim3(64), 0, s, a, sm, ch);
}

// one wavefront per tile of the planes, lane = pixel.  The record is read once, wave-uniform, and written by lane 0 after the tile's pixels:
// nobody else touches the tile, so the element-wise pass and the record update cannot race.
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

// one wavefront per tile of the planes: tile_rel_sum is adaptive_retire_kernel's body (noise_common.hpp); a tile with a record (retired, or any
// tile of budget mode) is priced with noise_var_retired
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
