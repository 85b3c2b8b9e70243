// evplp_path_trace_batch, first kernel of a chunk: primary visibility of the (active tile, sample) items into their staging slots.
//   pt_batch_primary_kernel  <- primary_kernel (kernels_trace.hip), one wavefront per item instead of per tile
// This translation unit is built like kernels_trace.hip, with -ffp-contract=off (Makefile): the texels must carry the bits evplp_primary
// gives them, and those depend on inlined helpers that no pragma inside the kernel reaches (primary_body.hpp).  That is also why the batch
// is two kernels in two translation units and not one fused kernel: the path tracer keeps contraction.
#include "device_common.hpp"
#include "kernels.h"

namespace evplp {

// item = blockIdx.x (kernels.h PtBatchChunk).  The packet walks start from the camera's entry cuts, which hold for every jitter up to a
// pixel (ch.cut_mask says which samples stay within that); the four texels of all 64 lanes go to the item's slot, nothing to the G-buffer
// planes.  The light plane gets the emitter colour where primary_kernel would put it under flags 0: every sample writes the same
// value, so concurrent items of one tile do not race.  a.clear_light is 0.
__global__ __launch_bounds__(64) void pt_batch_primary_kernel(PrimaryArgs a, PtBatchSamples sm, PtBatchChunk ch) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    const int item = (int)blockIdx.x;
    const int el = item / ch.sample_count, s = ch.sample_first + (item - el * ch.sample_count);
    const int e = ch.entry_first + el;
    const int n = ch.count ? *ch.count : ch.tiles;                   // (wave-uniform: scalar loads)
    if (e >= n) return;                                                   // the launch is sized from the tile total: surplus items
    const int tile = ch.list ? ch.list[e] : e;
    const int tiles_x = (a.st.W + 7) >> 3;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int x = tx * 8 + (lane & 7);
    const int ly = ty * 8 + (lane >> 3);
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

    float4 *slot = ch.staging + (size_t)item * 256 + lane;                // [plane][lane]: every store of the wave is one contiguous KB
    slot[0] = pos; slot[64] = nrm; slot[128] = dif; slot[192] = phg;
    if (in_image && light_visible) a.g_light[p] = make_float4(a.sc.light_unscaled[0], a.sc.light_unscaled[1], a.sc.light_unscaled[2], 0.f);
}

void launch_pt_batch_primary(const PrimaryArgs &a, const PtBatchSamples &sm, const PtBatchChunk &ch, hipStream_t s) {
    const long long items = (long long)ch.entry_count * ch.sample_count;
    if (items <= 0) return;
    hipLaunchKernelGGL(pt_batch_primary_kernel, dim3((unsigned)items), dim3(64), 0, s, a, sm, ch);
}

} // namespace evplp
