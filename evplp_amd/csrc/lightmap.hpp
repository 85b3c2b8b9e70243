// Lightmap baking (evplp_surface_points, evplp_lightmap_samples, evplp_bake_lightmap): the argument blocks of the kernels of
// kernels_lightmap.hip and their launchers.  The atlas is worked on in bands of whole texel rows that hold at most kLightmapChunk samples,
// so nothing the rasteriser allocates depends on width x height (include/evplp.h EVPLP_LIGHTMAP_CHUNK); the one array that is not bounded
// by a band is the tiles' triangle lists, which grow with the overlap of the scene's charts.
#pragma once
#include "evplp_types.h"
#include "kernels.h"
#include "lightmap_raster.h"

namespace evplp {

constexpr int32_t kLightmapChunk = EVPLP_LIGHTMAP_CHUNK;
constexpr int32_t kLightmapTile = 8;                       // a tile is 8 x 8 texels: one wave, lane = texel
static_assert(sizeof(evplp_lightmap_texel) == 32 && sizeof(evplp_hit) == 16 && sizeof(lm_tri) == 32, "a texel is two float4, a hit one, a set-up triangle two");
static_assert(kLightmapChunk >= LM_MAX_SIZE * 16, "a band holds at least one texel row of the widest atlas at 4 x 4 samples");

// hits -> surface points
struct PointsArgs {
    SceneDev sc;
    const evplp_hit *hits;        // [n]
    const float *eyes;            // [n][3] or null
    float4 *out;                  // [n][4]: evplp_surface_point
    int32_t n, ntris;             // ntris: the scene's ORIGINAL triangles (the attributes' count)
    uint32_t flags;
};

// the rasteriser.  The selection is the scene triangles [first, first + count); a band is the texel rows [y0, y0 + rows).
struct RasterArgs {
    const TriAttr *attrs;         // the scene's attributes (uvs == null: the selection's own texcoords)
    const float *uvs;             // [count][6] or null
    lm_tri *tris;                 // [count]: set up once per call
    int32_t first, count;
    int32_t width, height, samples;
    int32_t y0, rows;             // the band
    int32_t tiles_x, tiles;       // tiles of the band: tiles_x * ceil(rows / 8), numbered row by row
    uint32_t *counts;             // [tiles + 1]: triangles per tile (the last stays 0) ...
    uint32_t *offsets;            // [tiles + 1]: ... their exclusive sum: tile t's list is list[offsets[t] .. offsets[t + 1])
    uint32_t *cursors;            // [tiles]: the fill's
    uint32_t *list;               // [pairs]: indices into the selection, in no particular order (the winner is a minimum)
    uint32_t pairs;               // the list's capacity
    evplp_hit *out;               // the band's samples: index (((y - y0) * width + x) * S + j) * S + i
};

// a band's samples -> its texels
struct ResolveArgs {
    const float4 *points;         // [samples of the band][4]
    const float4 *lights;         // [samples of the band][2]: evplp_surface_light
    evplp_lightmap_texel *out;    // the band's first texel
    int32_t texels, s2;           // texels of the band, S * S
};
struct GutterArgs {
    const evplp_lightmap_texel *from; evplp_lightmap_texel *to;
    int32_t width, height, pass;  // pass d = 1 .. gutter
};

void launch_lightmap_points(const PointsArgs &a, hipStream_t s);
void launch_lightmap_setup(const RasterArgs &a, hipStream_t s);
size_t lightmap_scan_temp_bytes(int32_t tiles);                                 // the exclusive sum's workspace; 0: it states none
hipError_t launch_lightmap_count(const RasterArgs &a, void *temp, size_t temp_bytes, hipStream_t s);     // counts, then offsets
void launch_lightmap_fill_raster(const RasterArgs &a, hipStream_t s);            // the lists, then the band's samples
void launch_lightmap_resolve(const ResolveArgs &a, hipStream_t s);
void launch_lightmap_gutter(const GutterArgs &a, hipStream_t s);

}
