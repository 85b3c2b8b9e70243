// Probe gather (include/evplp.h "probe gather"): the host side of evplp_gather_probes and its device form.  A batch runs as launches of
// at most kProbeChunk probes (probe_gather.hpp), so the partial sums and the host form's staging have one size whatever n is; the kernels
// are in kernels_probe.hip.
#include "context.hpp"
#include "probe_gather.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace evplp;

namespace {
constexpr size_t kStagePositions = 3 * sizeof(float) * (size_t)kProbeChunk;          // the staged positions; the results lie behind them
constexpr size_t kStageBytes = kStagePositions + sizeof(evplp_probe_sh) * (size_t)kProbeChunk;
static_assert(kStagePositions % 16 == 0, "the staged results are written as float4");
constexpr size_t kMaxStackBytes = 64 * 1024;       // as ray_query.cpp: the largest dynamic LDS a workgroup may ask for without an attribute

int oom_or_hip(hipError_t e) { return e == hipErrorOutOfMemory ? EVPLP_ERR_OOM : EVPLP_ERR_HIP; }

// what both forms refuse, in evplp.h's order; ray_query_check serves for what the queries refuse as well
bool probe_check(evplp_context *c, const char *name, bool device, const evplp_probe_params *p, const void *positions, int32_t n, const void *out) {
    if (!ray_query_check(c, name, positions, n, 0, 0, out)) return false;
    if (!p) { c->set_error("%s: null params", name); return false; }
    if (!std::isfinite(p->min_distance) || !(p->min_distance > 0.0f)) { c->set_error("%s: min_distance %g is not a positive finite number", name, (double)p->min_distance); return false; }
    if (p->flags != 0u) { c->set_error("%s: unknown flag bits 0x%x", name, (unsigned)p->flags); return false; }
    if (p->num_vpl_light_paths == 0u || p->photons_per_path == 0u) { c->set_error("%s: num_vpl_light_paths or photons_per_path is 0", name); return false; }
    const uint64_t slots = (uint64_t)p->num_vpl_light_paths * p->photons_per_path, have = (uint64_t)c->cfg.num_light_paths * c->cfg.photons_per_path;
    if (slots > have) { c->set_error("%s: %llu record slots asked for, the context's record buffer holds %llu", name, (unsigned long long)slots, (unsigned long long)have); return false; }
    if (device && n > 0 && ((uintptr_t)out & 15u) != 0) { c->set_error("%s: the destination is not 16-byte aligned", name); return false; }
    return true;
}

// one batch, chunk by chunk.  device: positions / out are device pointers and nothing waits; else they are staged and every chunk is waited for.
int gather(evplp_context *c, const char *name, bool device, const evplp_probe_params *p, const void *positions, int32_t n, void *out) {
    if (!probe_check(c, name, device, p, positions, n, out)) return EVPLP_ERR_INVALID;
    if (n == 0) return EVPLP_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t lds = probe_stack_bytes(c->sc);
    if (lds > kMaxStackBytes) { c->set_error("%s: the walk's stack of this tree (%zu bytes per wave) exceeds a workgroup's LDS", name, lds); return EVPLP_ERR_INVALID; }
    const uint32_t slots = p->num_vpl_light_paths * p->photons_per_path;         // (checked against the record buffer: it fits 32 bits)
    const uint32_t slices = probe_slices(slots);
    hipError_t e = grow_scratch_of(c, c->probe_partial, probe_partial_bytes(slices));
    if (e != hipSuccess) { c->set_error("%s: cannot allocate the partial sums of %u slices (%zu bytes): %s", name, slices, probe_partial_bytes(slices), hipGetErrorString(e)); return oom_or_hip(e); }
    if (!device) {
        e = grow_scratch_of(c, c->probe_stage, kStageBytes);
        if (e == hipSuccess && !c->h_probe_stage) {
            e = hipHostMalloc((void **)&c->h_probe_stage, kStageBytes, hipHostMallocDefault);
            if (e != hipSuccess) { (void)hipGetLastError(); c->h_probe_stage = nullptr; }
        }
        if (e != hipSuccess) { c->set_error("%s: cannot allocate the staging of %d probes (%zu bytes): %s", name, kProbeChunk, kStageBytes, hipGetErrorString(e)); return oom_or_hip(e); }
    }
    for (int64_t at = 0; at < n; at += kProbeChunk) {
        const int32_t m = (int32_t)std::min<int64_t>(kProbeChunk, n - at);
        ProbeArgs a; std::memset(&a, 0, sizeof(a));
        a.sc = c->sc; a.records = (const evplp_record *)c->buf[EVPLP_BUF_RECORDS]; a.n = m; a.slots = slots; a.slices = slices;
        a.min_dist2 = p->min_distance * p->min_distance; a.paths = (float)p->num_vpl_light_paths;
        a.partial = (float *)c->probe_partial.p;
        if (device) { a.positions = (const float *)positions + 3 * (size_t)at; a.out = (evplp_probe_sh *)out + at; }
        else {
            std::memcpy(c->h_probe_stage, (const float *)positions + 3 * (size_t)at, 3 * sizeof(float) * (size_t)m);
            HIP_TRY(c, hipMemcpyAsync(c->probe_stage.p, c->h_probe_stage, 3 * sizeof(float) * (size_t)m, hipMemcpyHostToDevice, c->stream));
            a.positions = (const float *)c->probe_stage.p; a.out = (evplp_probe_sh *)((char *)c->probe_stage.p + kStagePositions);
        }
        launch_probe_gather(a, c->stream);
        launch_probe_reduce(a, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (!device) {
            HIP_TRY(c, hipMemcpyAsync(c->h_probe_stage + kStagePositions, a.out, sizeof(evplp_probe_sh) * (size_t)m, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            std::memcpy((evplp_probe_sh *)out + at, c->h_probe_stage + kStagePositions, sizeof(evplp_probe_sh) * (size_t)m);
        }
    }
    // (the overlapped light tracing may overwrite the records only behind their readers, as behind the gathers)
    if (c->aux_stream) HIP_TRY(c, hipEventRecord(c->ev_records_read, c->stream));
    return EVPLP_OK;
}
}

namespace evplp {
void release_probe_gather(evplp_context *c) {
    hipFree(c->probe_partial.p); hipFree(c->probe_stage.p); c->probe_partial = DeviceScratch(); c->probe_stage = DeviceScratch();
    if (c->h_probe_stage) hipHostFree(c->h_probe_stage);
    c->h_probe_stage = nullptr;
}
}

extern "C" int evplp_gather_probes(evplp_context *c, const evplp_probe_params *params, const float *positions, int32_t n, evplp_probe_sh *out) {
    CTX_CHECK(c);
    return gather(c, "evplp_gather_probes", false, params, positions, n, out);
}
extern "C" int evplp_gather_probes_device(evplp_context *c, const evplp_probe_params *params, const void *d_positions, int32_t n, void *d_out) {
    CTX_CHECK(c);
    return gather(c, "evplp_gather_probes_device", true, params, d_positions, n, d_out);
}
