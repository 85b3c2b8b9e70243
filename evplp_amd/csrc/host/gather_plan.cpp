// The launch plan of the VPL / VSL gathers (gather_plan.hpp): host only, no device, nothing but the standard library, like the deal of row
// blocks and the refit's level plan beside it (deal.cpp, refit_levels.cpp).  The results of a gather do not depend on any of it: the
// summation tree is fixed, and cuts, bands and group ranges only say where a walk starts and which launch runs it.
#include "gather_plan.hpp"

namespace evplp {
GatherPlan plan_gather(const GatherPlanInput &in) {
    GatherPlan p{};
    const bool small_launch = small_gather_launch(in.W, in.rows_in_image);
    // work-item size: k consecutive splits per wavefront.  A row strip of an n-way partition is a SMALL launch, and small launches want
    // short items: one rank's gather of an eight-way partition of config #2 takes 9.3 / 12.1 / 17.5 ms for k = 1 / 2 / 4 where an eighth of
    // the one-GPU kernel is 6.2 ms (profiles/r05_strip_projection.json); keyed on the size of the launch, not on strip_count > 1 (round 6: at
    // eight dealt ranks k = 2 projects x5.1 where k = 1 projects x6.5 -- an item twice as long is a tail twice as long).
    int k = in.splits_per_wave > 0 ? in.splits_per_wave : (small_launch ? 1 : kPlanDefaultSplitsPerWave);
    if (in.env_gather_k > 0) k = in.env_gather_k;
    // the per-item statistics need (VPLs per split) * k < 65536; the VSL estimator kernel's packed per-lane counters (VSLs per item) <= 4095
    const size_t per_split = in.nvpl_slots / kPlanVplSplit + 1;
    while (k > 1 && per_split * (size_t)k >= 65536) k >>= 1;
    if (in.vsl) while (k > 1 && per_split * (size_t)k > 4095) k >>= 1;
    if (in.vsl && per_split > 4095) { p.refused = "more than 4095 VSLs per item at k = 1: the estimator's packed counters would wrap"; return p; }
    p.k = k; p.groups = kPlanVplSplit / k;
    // tiles to XCDs while an XCD's share is >= 1024 tiles (its sum of tile costs then averages out: 1.9 % spread at 1024 x 1024), items over
    // all XCDs below that (a strip of an n-way partition, small images); EVPLP_ITEM_DEAL=0 / 1 forces either (developer A/B)
    p.item_deal = in.env_item_deal >= 0 ? in.env_item_deal : (small_launch ? 1 : 0);
    // tile blocks: as many tile rows as a row strip keeps adjacent, at most 8; EVPLP_TILE_BLOCK_LOG2 lowers it (0 = rows of 8 tiles)
    int sh = 8;
    if (in.strip_count > 1) { sh = 1; while (sh * 2 <= std::min(8, in.strip_rows / 8) && (in.strip_rows / 8) % (sh * 2) == 0) sh *= 2; }
    p.block_h_log2 = sh == 8 ? 3 : sh == 4 ? 2 : sh == 2 ? 1 : 0;
    if (in.env_tile_block_log2 >= 0) p.block_h_log2 = std::min(in.env_tile_block_log2, p.block_h_log2);
    sh = 1 << p.block_h_log2;
    p.tiles_y = (in.local_rows + 7) / 8; p.nby = (p.tiles_y + sh - 1) / sh;
    p.band_rows = p.nby; p.nbands = p.nby > 0 ? 1 : 0;
    // entry cuts (kernels.h CutArgs): one slot per (tile group, VPL slot), groups of 2 x 2 tiles where a block has two tile rows that are
    // neighbours in the image, 2 x 1 otherwise.  The scratch holds as many rows of tile blocks as fit its bound, and a frame with more is
    // gathered band by band; a bound below one row of tile blocks (or no scratch at all) leaves one band whose walks start at the root.
    if (in.env_cuts != 0 && in.cuts_available && p.nby > 0) {
        const int gh_log2 = (sh >= 2 && tile_rows_are_neighbours(in.strip_count, in.strip_rows)) ? 1 : 0, groups_x = ((in.W + 7) / 8 + 1) >> 1;
        const size_t per_block_row = (size_t)(sh >> gh_log2) * (size_t)groups_x * (uint32_t)in.nvpl_slots * (size_t)kPlanCutSlotBytes;
        const int band_rows = (int)std::min<size_t>((size_t)p.nby, in.cut_cap / std::max<size_t>(per_block_row, 1));
        if (band_rows >= 1) {
            p.use_cuts = true; p.gw_log2 = 1; p.gh_log2 = gh_log2; p.groups_x = groups_x; p.vpl_stride = (uint32_t)in.nvpl_slots;
            p.band_rows = band_rows; p.nbands = (p.nby + band_rows - 1) / band_rows; p.cut_bytes = per_block_row * (size_t)band_rows;
        }
    }
    p.groups_per_launch = p.groups; p.group_launches = 1;
    if (in.vsl) {
        // lit masks between the walk and the estimator kernel: 8 bytes per (tile, VSL slot) of a launch, sized for the first band (no band
        // has more tiles); the groups of a tile are covered in as many launches as keep the buffer within its bound
        p.masks_per_split = (int32_t)((in.nvpl_slots + kPlanVplSplit - 1) / kPlanVplSplit);
        const size_t tiles = (size_t)gather_band_tiles(in.W, in.local_rows, p.block_h_log2, 0, p.nbands > 1 ? p.band_rows : 0);
        const size_t per_item = (size_t)k * (size_t)p.masks_per_split * sizeof(unsigned long long);
        while (p.groups_per_launch > 1 && tiles * (size_t)p.groups_per_launch * per_item > in.mask_cap) p.groups_per_launch = (p.groups_per_launch + 1) / 2;
        p.group_launches = (p.groups + p.groups_per_launch - 1) / p.groups_per_launch;
        p.mask_bytes = tiles * (size_t)p.groups_per_launch * per_item;
    }
    return p;
}

GatherBand gather_band(const GatherPlan &p, int i) {
    GatherBand b{};
    b.first = i * p.band_rows; b.rows = std::min(p.band_rows, p.nby - b.first); b.args_rows = p.nbands > 1 ? b.rows : 0;
    if (p.use_cuts) {       // (a block is a whole number of group rows: gh_log2 = 1 only under blocks of two tile rows and more)
        const int sh = 1 << p.block_h_log2, g = p.gh_log2, groups_total_y = (p.tiles_y + (1 << g) - 1) >> g;
        b.group_row_first = (b.first * sh) >> g;
        b.groups_y = std::min(((b.first + b.rows) * sh + (1 << g) - 1) >> g, groups_total_y) - b.group_row_first;
    }
    return b;
}

GatherGroupRange gather_group_range(const GatherPlan &p, int j) {
    const int first = j * p.groups_per_launch;
    return { first, std::min(p.groups_per_launch, p.groups - first) };
}
}
