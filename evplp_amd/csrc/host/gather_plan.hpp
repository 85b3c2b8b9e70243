// host/gather_plan.cpp: how a VPL / VSL gather (context.cpp run_gather) cuts a frame into launches -- splits per wavefront, item deal, tile
// blocks, cut groups, bands of tile-block rows under the cut-scratch bound, group ranges under the VSL mask bound.  A pure function of a few
// integers: no device, no context, nothing but the standard library (tools/host_fuzz/gather_plan_check.cpp checks it without a GPU).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace evplp {
#pragma GCC visibility push(hidden)
// kernels.h kVplSplit, kDefaultSplitsPerWave and kCutSlotBytes, restated because this unit sees no HIP header (context.cpp asserts that they agree)
constexpr int kPlanVplSplit = 128, kPlanDefaultSplitsPerWave = 2, kPlanCutSlotBytes = 256;

// ---- the rules that more than one place follows, each stated here and nowhere else
// a strip's tile rows are neighbours in the image (one GPU, or strips of 16 rows and more): the gather's and the eye's cut groups are then
// 2 x 2 tiles, 2 x 1 otherwise
inline bool tile_rows_are_neighbours(int strip_count, int strip_rows) { return strip_count == 1 || strip_rows >= 16; }
// a small launch: at most 8 192 OWNED tiles -- half a 1024 x 1024 image, a rank of a two-way partition (the capacity rows a dealt partition
// keeps in reserve hold nothing and leave at once).  Small launches want short items (k = 1) dealt over all XCDs.
inline bool small_gather_launch(int W, int rows_in_image) { return (size_t)((W + 7) / 8) * (size_t)((rows_in_image + 7) / 8) <= 8192; }
// VPL record slots of a context: d_vpls, d_vpl_src and every (tile group, VPL) row of the cut scratch are this long
inline size_t nvpl_slot_count(uint32_t num_vpl_light_paths, uint32_t photons_per_path) { return std::max<size_t>((size_t)num_vpl_light_paths * photons_per_path, 1); }
// tiles a gather launch enumerates: whole blocks of 8 x (1 << block_h_log2) tiles over the rows [band_first, band_first + band_rows) of
// tile blocks (band_rows = 0: all of them).  kernels_gather.hip's grid is this count times the launch's groups.
inline int gather_band_tiles(int W, int local_rows, int block_h_log2, int band_first, int band_rows) {
    const int tiles_x = (W + 7) / 8, tiles_y = (local_rows + 7) / 8, sh = 1 << block_h_log2;
    const int nby = (tiles_y + sh - 1) / sh, rows = band_rows > 0 ? std::min(band_rows, nby - band_first) : nby;
    return ((tiles_x + 7) / 8) * std::max(rows, 0) * 8 * sh;
}

struct GatherPlanInput {
    int32_t W, local_rows, rows_in_image, strip_count, strip_rows;      // the context's share of the frame (StripDev)
    size_t nvpl_slots;                  // nvpl_slot_count
    bool vsl;                           // evplp_gather_vsl: the estimator's counter limit, the lit masks
    int32_t splits_per_wave;            // evplp_config.gather_splits_per_wave (0: automatic)
    int32_t env_gather_k, env_item_deal, env_tile_block_log2, env_cuts;     // the context's overrides (0 / -1 / -1 / -1: not set)
    size_t cut_cap, mask_cap;           // bounds of the cut scratch and of the VSL mask buffer, in bytes
    bool cuts_available;                // false: plan without entry cuts (the caller could not allocate cut_bytes)
};
struct GatherPlan {
    const char *refused;                // null, or why there is no plan (nothing else is filled then)
    int32_t k, groups;                  // splits per wavefront; groups of a tile = kPlanVplSplit / k
    int32_t item_deal, block_h_log2;    // GatherArgs of the same names
    int32_t tiles_y, nby;               // tile rows; rows of tile blocks
    bool use_cuts;                      // the walks start from entry cuts (else from the root, and the next five are 0)
    int32_t gw_log2, gh_log2, groups_x; uint32_t vpl_stride; size_t cut_bytes;       // CutArgs; what the cut scratch must hold (one band's slots)
    int32_t band_rows, nbands;          // rows of tile blocks per band (the last may have fewer); bands
    int32_t masks_per_split, groups_per_launch, group_launches;      // VSL (0 / groups / 1 otherwise): a band's groups go in that many launches
    size_t mask_bytes;                  // what the mask buffer must hold: the first band's tiles x groups_per_launch
};
GatherPlan plan_gather(const GatherPlanInput &in);

// band i: rows [first, first + rows) of tile blocks and, with cuts, rows [group_row_first, group_row_first + groups_y) of tile groups;
// args_rows: what GatherArgs::band_rows takes -- rows, or 0 ("all") when the plan is a single band
struct GatherBand { int32_t first, rows, args_rows, group_row_first, groups_y; };
GatherBand gather_band(const GatherPlan &p, int i);
// group launch j of a band: the groups [first, first + count) of every tile
struct GatherGroupRange { int32_t first, count; };
GatherGroupRange gather_group_range(const GatherPlan &p, int j);
#pragma GCC visibility pop
}
