// Probe gather (evplp_gather_probes): the argument block of its two kernels and their launchers (kernels_probe.hip).  A launch takes at
// most kProbeChunk probes: that bounds the partial sums and the host form's staging for any batch (include/evplp.h EVPLP_PROBE_CHUNK).
#pragma once
#include "evplp_types.h"
#include "kernels.h"

namespace evplp {

constexpr int32_t kProbeChunk = EVPLP_PROBE_CHUNK;
constexpr uint32_t kProbeSlice = EVPLP_PROBE_SLICE_SLOTS;
constexpr int kProbeFloats = sizeof(evplp_probe_sh) / sizeof(float);      // 27 coefficients and lit
static_assert(sizeof(evplp_probe_sh) == 112 && kProbeFloats == 28, "the reduce writes a probe as seven float4");
static_assert(kProbeChunk % 64 == 0, "a chunk is whole waves");

struct ProbeArgs {
    SceneDev sc;
    const float *positions;       // [n][3]
    const evplp_record *records;  // [slots]
    int32_t n;                    // probes of this launch, <= kProbeChunk
    uint32_t slots, slices;       // slices = ceil(slots / kProbeSlice)
    float min_dist2, paths;       // min_distance^2, (float)num_vpl_light_paths
    float *partial;               // [slices][kProbeFloats][kProbeChunk]: a slice's sums of probe i at ((slice * 28 + f) * kProbeChunk + i)
    evplp_probe_sh *out;          // [n]
};
inline uint32_t probe_slices(uint64_t slots) { return (uint32_t)((slots + kProbeSlice - 1) / kProbeSlice); }
inline size_t probe_partial_bytes(uint32_t slices) { return (size_t)kProbeChunk * slices * sizeof(evplp_probe_sh); }
// dynamic LDS of the gather kernel: the occlusion walk's full [entry][lane] stack (kernels.h lane_stack_bytes4)
size_t probe_stack_bytes(const SceneDev &sc);
void launch_probe_gather(const ProbeArgs &a, hipStream_t s);      // one wave per (64 probes, slice) -> partial
void launch_probe_reduce(const ProbeArgs &a, hipStream_t s);      // partial -> out

}
