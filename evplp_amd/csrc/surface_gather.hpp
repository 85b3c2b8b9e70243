// Surface gather (evplp_gather_surface): the argument blocks of its kernels and their launchers (kernels_surface.hip).  A launch takes at
// most kSurfaceChunk points: that bounds the partial sums and the host form's staging for any batch (include/evplp.h EVPLP_SURFACE_CHUNK).
// The photon grid is built once per call over the record slots, whatever n is.
#pragma once
#include "evplp_types.h"
#include "kernels.h"

namespace evplp {

constexpr int32_t kSurfaceChunk = EVPLP_SURFACE_CHUNK;
constexpr uint32_t kSurfaceSlice = EVPLP_PROBE_SLICE_SLOTS;        // the probe gather's decomposition
constexpr int kSurfaceCompactF4 = 5;                               // float4 per photon of the grid's compact record
static_assert(sizeof(evplp_surface_point) == 64 && sizeof(evplp_surface_light) == 32, "a point is four float4, a result two");
static_assert(kSurfaceChunk % 64 == 0, "a chunk is whole waves");

// the grid of one call: photon_grid.h's plan over the scene's box, and the arrays the build leaves for the query
struct SurfaceGrid {
    float lo[3], hi[3];           // the scene's box
    float edge, radius;
    uint32_t bits, slots;         // 2^bits buckets; record slots [0, slots) were looked at
    const uint32_t *start;        // [2^bits + 2]: bucket b is compact[start[b] .. start[b + 1]); bucket 2^bits holds the unusable slots
    const float4 *compact;        // [slots][kSurfaceCompactF4], sorted by (bucket, slot): [0] pos, cpn  [1] w12, d2  [2] wflux, alive  [3] brdf2  [4] cell, slot
};
// what the build writes, in the order it runs
struct SurfaceGridBuild {
    SurfaceGrid g;
    evplp_frame_params fp;
    const evplp_record *records;
    uint32_t *keys, *keys_sorted, *vals, *vals_sorted, *start;
    float4 *compact;
    void *temp; size_t temp_bytes;
};

struct SurfaceArgs {
    SceneDev sc;
    evplp_frame_params fp;        // mis_mode, pdf_mc, clamping_value, photon_radius, the counts; camera_pos where eyes is null
    const float4 *points;         // [n][4]: evplp_surface_point
    const float *eyes;            // [n][3] or null
    const evplp_record *records;
    int32_t n;                    // points of this launch: <= kSurfaceChunk for the VPL half and the reduce; the photon query takes any number
    uint32_t what;
    uint32_t slots, slices;       // the VPL half: slices = ceil(slots / kSurfaceSlice)
    float pdf_mc2, paths;         // pdf_mc^2, (float)num_vpl_light_paths
    float *partial;               // [slices][4][kSurfaceChunk]: a slice's r, g, b, lit of point i at ((slice * 4 + f) * kSurfaceChunk + i)
    evplp_surface_light *out;     // [n]
    SurfaceGrid grid;
};
inline uint32_t surface_slices(uint64_t slots) { return (uint32_t)((slots + kSurfaceSlice - 1) / kSurfaceSlice); }
inline size_t surface_partial_bytes(uint32_t slices) { return (size_t)kSurfaceChunk * (size_t)(slices ? slices : 1u) * 4 * sizeof(float); }
size_t surface_stack_bytes(const SceneDev &sc);                    // dynamic LDS of the VPL kernel (kernels.h lane_stack_bytes4)
size_t surface_sort_temp_bytes(uint32_t slots, uint32_t bits);     // the radix sort's workspace; 0: it states none
hipError_t launch_surface_grid(const SurfaceGridBuild &b, hipStream_t s);   // cells and keys, the stable sort, bucket starts, compact records
void launch_surface_vpl(const SurfaceArgs &a, hipStream_t s);      // one wave per (64 points, slice) -> partial
void launch_surface_photons(const SurfaceArgs &a, hipStream_t s);  // lane = point -> the second half of out
void launch_surface_reduce(const SurfaceArgs &a, hipStream_t s);   // partial -> the first half of out

// The progressive gather (evplp_gather_surface_progressive; kernels_surface_prog.hip).  The VPL half and the grid build are the kernels
// above; the new unit rewrites the compact records' flux without InvPi / r^2, walks with the lane's own radius into the lane's state,
// folds the reduced VPL half in, and resolves.
static_assert(sizeof(evplp_surface_state) == 48, "a state is three float4");
struct SurfaceProgArgs {
    evplp_frame_params fp;        // mis_mode (0, 4, 5), clamping_value, photon_radius, num_light_paths; camera_pos where eyes is null
    const float4 *points;         // [n][4]
    const float *eyes;            // [n][3] or null
    const float4 *lights;         // [n][2]: the reduce's evplp_surface_light of this launch (the fold reads the first 16 bytes)
    float4 *states;               // [n][3]: evplp_surface_state, in and out
    int32_t n;                    // <= kSurfaceChunk for the fold; the query and the resolve take any number
    uint32_t what;
    float alpha, r0sq;            // r0sq = fl(photon_radius * photon_radius)
    SurfaceGrid grid;
};
struct SurfaceResolveArgs { const float4 *states; float4 *out; int32_t n; };     // [n][3] -> [n][2]
// states of an atlas -> its texels (evplp_bake_lightmap_resolve): lane = texel over its s2 samples' states
struct LightmapProgResolveArgs { const float4 *states; evplp_lightmap_texel *out; int32_t texels, s2; };
void launch_surface_prog_compact(const SurfaceGridBuild &b, hipStream_t s);      // behind launch_surface_grid: wflux = flux / num_light_paths
void launch_surface_prog_fold(const SurfaceProgArgs &a, hipStream_t s);
void launch_surface_prog_photons(const SurfaceProgArgs &a, hipStream_t s);
void launch_surface_prog_resolve(const SurfaceResolveArgs &a, hipStream_t s);
void launch_lightmap_prog_resolve(const LightmapProgResolveArgs &a, hipStream_t s);

// The k-nearest-photon start radius (evplp_gather_surface_knn; kernels_surface_knn.hip).  The grid and the compact records are the
// progressive gather's; the select leaves a squared radius per point of the launch, the photon kernel seeds the fresh states with it.
struct SurfaceKnnArgs {
    SurfaceProgArgs p;            // fp, points, eyes, states, n (any number), alpha, r0sq, grid; lights and what are not read
    float *rk2;                   // [n]: written by the select and read by the photon kernel, for the lanes both decide to be this call's
    uint32_t k;                   // >= 1
    float rminsq;                 // fl(r_min * r_min), within [2^-100, r0sq]
};
void launch_surface_knn_select(const SurfaceKnnArgs &a, hipStream_t s);          // lane = point -> rk2
void launch_surface_knn_photons(const SurfaceKnnArgs &a, hipStream_t s);         // lane = point: the first photon half at rk2 -> states

}
