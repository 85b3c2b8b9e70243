// evplp_path_trace_batch (kernels.h PtBatchChunk), the kernel that must round every operation on its own: this unit is built like
// kernels_trace.hip, with -ffp-contract=off (Makefile).  The texels must carry the bits evplp_primary gives them, and those depend on inlined
// helpers that no pragma inside the kernel reaches (primary_body.hpp).  That is also why a chunk is two kernels in two translation units and
// not one fused kernel: the path tracer keeps contraction.
//   pt_batch_primary_kernel   <- primary_kernel (kernels_trace.hip), one wavefront per item of the table instead of per tile
// (budget mode's per-tile fold and per-tile noise figure: kernels_stats.hip)
#include "device_common.hpp"
#include "kernels.h"

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

} // namespace evplp
