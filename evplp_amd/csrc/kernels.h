// Kernel argument blocks and host-side launchers (defined in the .hip files).
#pragma once
#include "evplp_types.h"

namespace evplp {

struct PrimaryArgs {
    SceneDev sc; StripDev st; CamBasis cam;
    float jitter[2]; int32_t clear_light; int32_t pad;
    float4 *g_pos, *g_nrm, *g_dif, *g_phg, *g_light;
    float4 *tile_box;         // [tiles][2] world-space box of every 8x8-px tile's positions (the photon splat's bin cull), or null
    // entry cuts of the primary rays (one slot per tile group, built once per camera by primary_cut_kernel; null: walks from the root)
    const char *cuts; int32_t cut_gw_log2, cut_gh_log2, cut_groups_x, pad2;
};
// The eye's entry cuts: the pyramid through a tile group's pixels -- opened by one pixel on every side, so that it holds for every
// anti-aliasing jitter of the camera -- descends the tree like a (tile group, VPL) pyramid (CutArgs below); lane = tile group.
struct PrimaryCutArgs {
    const BvhNode *nodes; StripDev st; CamBasis cam;
    int32_t tiles_x, tiles_y, gw_log2, gh_log2, groups_x, groups_y;
    char *cuts;
};
void launch_primary_cuts(const PrimaryCutArgs &a, hipStream_t s);
// the deal of primary_kernel's tiles to workgroups (kernels_trace.hip; prev_pose_kernel, kernels_temporal.hip, follows it)
#ifndef EVPLP_PRIMARY_BLOCKS
#define EVPLP_PRIMARY_BLOCKS 1
#endif
#ifndef EVPLP_PRIMARY_BLOCK_LOG2
#define EVPLP_PRIMARY_BLOCK_LOG2 2     // 4 x 4 tiles
#endif

struct LightTraceArgs {
    SceneDev sc;
    uint32_t rng_seed, path_begin, path_count, photons_per_path;
    evplp_record *records;
    int32_t *stack_overflow;      // [lt_overflow_entries(sc)][path_count rounded up to 64]: the walk's stack beyond its LDS entries
    uint32_t overflow_stride, pad;
};
#ifndef EVPLP_LT_STACK
#define EVPLP_LT_STACK 20
#endif
constexpr int kLtLdsStack = EVPLP_LT_STACK;   // LDS entries of light tracing's walk stack (20: 5 KB per wave); the rest of the worst case lives in global memory
inline int lt_overflow_entries(const SceneDev &sc) {
    const int generic = 3 * ((sc.bvh_depth + 1) / 2) + 4;
    const int worst = sc.stack4_entries > 0 && sc.stack4_entries < generic ? sc.stack4_entries : generic;
    return worst > kLtLdsStack ? worst - kLtLdsStack : 0;
}

// Device-side counters of one pass (zeroed by the host before the launch)
struct PassCounters {
    unsigned long long rays;          // shadow / closest-hit rays actually traced
    unsigned long long nodes;         // BVH nodes visited (wave-level visits for the gather)
    unsigned long long pairs;         // splat: (photon, pixel) pairs inside the kernel radius
    unsigned long long aux;
    // EVPLP_TRAVERSAL_STATS builds only (tools/traversal_stats.py): histogram of leaf blocks tested per (wave, VPL) walk
    // ([31] = 31 or more), [32] = walks, [33] = triangle pairs tested, [34] = walks that ended with every lane occluded,
    unsigned long long hist[64];
    // gather: shadow rays / unoccluded pairs, summed by gather_reduce_kernel into 64 shards (one device-scope atomic per
    // workgroup; a single word saturates near 90 atomics per microsecond)
    unsigned long long shard_rays[64], shard_shaded[64];
    // -DEVPLP_DEBUG_NAN builds only (`make nan`): pixels whose partial sum / splat sum came out non-finite -- the reference's ASSERT under
    // DEBUG (realtimetechniques/all.cuh:10-17) as a counter (word 196 of evplp_debug_counters)
    unsigned long long nonfinite;
};
#ifndef EVPLP_DEBUG_NAN
#define EVPLP_DEBUG_NAN 0
#endif
constexpr int kCounterShards = 64;

struct GatherArgs {
    SceneDev sc; StripDev st;
    const float4 *g_pos, *g_nrm, *g_dif, *g_phg;
    const evplp_record *vpls;         // compacted usable VPL records
    const uint32_t *vpl_src_index;    // VSL only: original record index of each compacted VPL (RNG substream)
    const uint32_t *nvpl;             // device scalar written by compact_vpl_kernel
    evplp_frame_params fp;
    float pdf_mc2; int32_t pad0;      // fp.pdf_mc squared (power2 heuristic)
    float4 *out;
    float4 *partial;                  // [kVplSplit / splits_per_wave][partial_stride] per-item partial sums
    size_t partial_stride;            // W * local_rows
    PassCounters *counters;
    int32_t splits_per_wave;          // k: a wave sums k consecutive splits (a power of two <= 32) and folds them in tree order
    int32_t block_h_log2;             // tiles are enumerated in blocks of 8 x (1 << block_h_log2) tiles
    // a launch covers the groups [group_first, group_first + group_count) of every tile (group_count = 0: all 128 / k of them)
    int32_t group_first, group_count;
    // VSL gather (two kernels): lit-lane masks of every (item, VSL) of the launch, [item][k * masks_per_split], written by
    // gather_vsl_walk_kernel and read by gather_vsl_shade_kernel
    unsigned long long *vsl_masks; int32_t masks_per_split; int32_t pad1;
    // entry cuts (round 4, CutArgs below): the walks of tile (tx, ty) for VPL i start from the cut of its tile group, at
    // cuts + ((group index) * cut_vpl_stride + i) * kCutSlotBytes; null = walks start at the root
    const char *cuts; uint32_t cut_vpl_stride; int32_t cut_gw_log2, cut_gh_log2, cut_groups_x;
    // a launch covers the rows [band_first, band_first + band_rows) of tile BLOCKS only (band_rows = 0: all of them): the entry cuts of a
    // large configuration are built and consumed band by band so that their scratch stays bounded (config #5: 137 GB for all at once).
    // cut_group_row_first: the first row of tile groups that has slots in `cuts`
    int32_t band_first, band_rows, cut_group_row_first;
    int32_t item_deal;                // 1: a tile's items go to all XCDs (small launches: strips); 0: tiles are dealt to XCDs (kernels_gather.hip item_index)
    // calibration launches only (evplp_calibrate_blocks; the kernels' COST variants): the 100 MHz clock ticks every item was resident, added to
    // its local block's counter -- what evplp_group_rebalance deals the blocks by
    unsigned long long *block_cost;
};
// evplp_adaptive_enable: the gather kernels' last argument (read by their ADAPT variants only; tiles = null: adaptivity is off) -- the tile
// records of the context's planes [tiles_x * tiles_y] (AdaptTiles below), the retired pixels' snapshot of VPL_ACCUM [W * local_rows], and
// N + 1 (N: the accumulating gather calls before this one).  (A separate argument: GatherArgs, and with it every default kernel, stays as it was.)
struct AdaptArgs { const int4 *tiles; const float4 *snap; int32_t n1, pad; };
// Entry cuts.  A frustum around ALL segments between one VPL and the pixels of a group of 2 x 2 tiles (the box of their end points
// + four planes through the VPL) descends the tree breadth-first, dropping every subtree it cannot reach, until the surviving cut
// would exceed kCutEntries; the group's (tile, VPL) packet walks then start from the cut -- two cut entries per synthetic node, in
// the BvhNode format, so the walk's node visit tests them -- instead of from the root.  Measured on the walk population of the
// bench configuration with the CPU replay (tools/bvh_eval/walk_proxy.cpp): 34.8 -> 16.0 node visits per walk, half of the walks
// start from an empty cut; 8.7 frustum steps per tile walk at ~1.5 vector instructions per step and lane.
constexpr int kCutEntries = 8;                     // cut entries per (group, VPL): 17.6 node visits per walk in the CPU replay against 16.9 with 16 entries, for a quarter fewer descent steps, half the slot and half as many synthetic visits
constexpr int kCutNodes = kCutEntries / 2;         // synthetic nodes per slot
constexpr int kCutSlotBytes = kCutNodes * 64;
struct CutArgs {
    const BvhNode *nodes;
    const float4 *tile_box;           // [tiles][2] world-space box of every tile's G-buffer positions (primary_kernel / tile_box_kernel)
    int32_t tiles_x, tiles_y;         // tiles of this context's strip
    int32_t gw_log2, gh_log2;         // tiles per group: 2 x 2 (2 x 1 when the strip's tile rows are not neighbours in the image)
    int32_t groups_x, groups_y;       // groups per row; rows of groups of THIS launch
    int32_t group_row_first, pad;     // first row of groups of this launch (slot 0 of `cuts` belongs to its first group)
    const evplp_record *vpls; const uint32_t *nvpl; uint32_t vpl_stride;     // compacted usable VPLs; slots per group in `cuts`
    char *cuts;
    const int4 *adapt_tiles;          // non-null: skip the groups whose tiles are all retired (evplp_adaptive_retire; tile records as GatherArgs)
};
void launch_gather_cuts(const CutArgs &a, hipStream_t s);
void launch_tile_boxes(const StripDev &st, const float4 *g_pos, float4 *tile_box, int tiles_x, int tiles_y, hipStream_t s);
#ifndef EVPLP_VPL_SPLIT
#define EVPLP_VPL_SPLIT 128
#endif
// VPL i belongs to split i % kVplSplit; a pixel's sum is the balanced binary tree over the kVplSplit per-split sums, each
// split summed in increasing i.  A constant, and a fixed tree: results must not depend on the GPU count or on splits_per_wave.
constexpr int kVplSplit = EVPLP_VPL_SPLIT;
#ifndef EVPLP_GATHER_K
#define EVPLP_GATHER_K 2
#endif
// (round 4) k = 2: with the entry cuts an item of four splits is long against its set-up again (k = 2 / 4 / 8: 57.6 / 58.6 / 71.1 ms);
// 64 partial sums per pixel, 1 GB at 1024^2.  Rounds 1-3, k = 4: 32 partial sums per pixel (512 MB at 1024^2 instead of 2 GB for k = 1) at the same speed (hard scene, cfg2, one GPU:
// k = 1 113.9 ms, 2 114.3, 4 114.0 on one box); k = 16 was 38 % slower (long items: launch tail)
constexpr int kDefaultSplitsPerWave = EVPLP_GATHER_K;
#ifndef EVPLP_PX_LDS
#define EVPLP_PX_LDS 1            // the pixel's reflectances parked in LDS beside its view direction: seven registers fewer across the walks
#endif
constexpr int kGatherPxFloats = 64 * (EVPLP_PX_LDS ? 10 : 3);      // [192] view direction (+ [192] rho_d, [192] rho_s, [64] e) per wavefront
// Dynamic LDS of a gather wavefront that folds its k split sums (a power of two) in tree order: `px_floats` of pixel data, then one
// [3][64] block per fold level.  A binary counter over k splits has log2 k + 1 levels; the top one only ever receives the last split's
// store, which nothing reads back: a kernel that skips that store (gather_vpl_kernel) asks with top_level = false.
constexpr size_t gather_fold_lds_bytes(int k, int px_floats, bool top_level) {
    int levels = 1;
    while ((1 << (levels - 1)) < k) levels++;       // log2 k + 1
    return (size_t)((top_level ? levels : levels - 1) * 192 + px_floats) * sizeof(float);
}
// ... of gather_vpl_kernel: what launch_gather_vpl_items asks for (tests/test_gather_ring_resources.py adds the kernel's static ring to it)
constexpr size_t gather_vpl_lds_bytes(int k) { return gather_fold_lds_bytes(k, kGatherPxFloats, false); }

struct PathTraceArgs {
    SceneDev sc; StripDev st;
    const float4 *g_pos, *g_nrm, *g_dif, *g_phg;
    float camera_pos[3]; uint32_t rng_seed;
    uint32_t max_bounces, do_accumulate;
    float4 *out;
    PassCounters *counters;
};

// evplp_path_trace_batch: S complete iterations (primary visibility + one camera path) in one call, every tile taking its own number of them
// (pt_tile_samples below).  The work is an ITEM TABLE, one item per (tile, sample), one wavefront each, lane = pixel, so a thin tail of noisy
// tiles still fills the machine: pt_batch_scan_kernel walks the tiles in increasing index and writes first[t], the exclusive prefix sum of the
// tiles' counts (first[tiles] = the total); pt_batch_fill_kernel writes table[first[t] + s] = t * 64 + s.  A tile's samples are consecutive
// items, so the workgroup dispatcher's round-robin deals them over all eight XCDs (as the gather's item_deal = 1 does for small launches).
// An item owns one staging SLOT, [4 planes][64 lanes] float4: the batched primary writes the sample's four texels there, the batched trace
// reads them and puts (r, g, b, valid) of the sample into plane 0, and pt_batch_accumulate_kernel adds the chunk's part of
// [first[t], first[t + 1]) to the tile's pixels one sample at a time in increasing s -- the order of S single calls -- in VPL_ACCUM, or in
// budget mode in the snapshot plane, where the tile's raw sum R lives.  Once per call pt_batch_close_kernel writes the pixels that are an
// extrapolation: mode 1, the retired tiles' as (float)(R * ((N + S) / n_t)); mode 2, n_t += s_t and every tile's as (float)(R * (N / n_t)).
constexpr int kPtBatchMaxSamples = 64;
constexpr int kPtBatchMaxTiles = 1 << 25;                          // tile * 64 + s in 32 bits: evplp_path_trace_batch refuses a context with more
constexpr size_t kPtBatchSlotBytes = 4 * 64 * sizeof(float4);      // 64 B per pixel-sample
struct PtBatchSamples { float jitter[kPtBatchMaxSamples][2]; uint32_t seed[kPtBatchMaxSamples]; };
// The samples 0 .. s_t - 1 of a call of S that the tile with record r takes: the scan kernel's count and the host's (staging and table sizes,
// budget mode's n_t).  mode 0, adaptivity off (no records, r is ignored): S.  Mode 1 (evplp_adaptive_enable_pt(ctx, 1), r = { n_t, K_t, B_t, 0 }):
// S for an active tile, 0 for a retired one.  Mode 2, budget mode (r = { n_t, K_t, B_t, b_t }): the budget, -1 = all.
__host__ __device__ inline int32_t pt_tile_samples(int32_t mode, int4 r, int32_t S) {
    return mode == 0 ? S : mode == 1 ? (r.x == 0 ? S : 0) : (r.w < 0 || r.w > S ? S : r.w);
}
// Gather budget mode (evplp_adaptive_enable(ctx, 2), r = { n_t, K_t, B_t, b_t }): does the tile take the accumulating gather call at `phase` =
// m % S of its window of S calls?  The first min(b_t, S) calls of every window, -1 = all: the mask kernel's rule and the host's (n_t).
__host__ __device__ inline bool gather_tile_takes(int4 r, int32_t phase, int32_t S) {
    return r.w < 0 || phase < (r.w < S ? r.w : S);
}
constexpr int kGatherBudgetMaxWindow = 64;
// The mode's three kernels (kernels_gather.hip).  mask[t] = { takes ? 0 : max(n_t, 1), takes, 0, 0 }: .x is what the gathers' ADAPT variants and
// the cut kernel read in place of the records, so a skipping tile looks retired to them for this call; .y is what the reduce and the step read.  The reduce writes R = reduce_out(tree, .., R) into the
// snapshot plane for the written pixels of a taking tile and VPL_ACCUM = extrapolate(R, n1, n_t + takes) for every in-image pixel; the step
// kernel then does n_t += takes (one thread per tile, after the reduce: a tile's pixels lie in several of the reduce's workgroups).
void launch_gather_budget_mask(const int4 *tiles, int32_t ntiles, int32_t phase, int32_t window, int4 *mask, hipStream_t s);
void launch_gather_budget_step(int4 *tiles, const int4 *mask, int32_t ntiles, hipStream_t s);
void launch_gather_reduce_budget(const GatherArgs &a, int stencil_test, const int4 *tiles, const int4 *mask, float4 *snap, int32_t n1, hipStream_t s);
// one chunk of a call: the items [item_first, item_first + item_count), slot = item - item_first; items at or beyond the total exit
struct PtBatchChunk {
    const uint32_t *table; const int32_t *total;
    int32_t item_first, item_count;
    float4 *staging;                  // [item_count] slots
    unsigned long long cut_mask;      // bit s: sample s's jitter lies within the eye's entry cuts (evplp_primary's test); else it walks from the root
};
void launch_pt_batch_table(const int4 *tiles, int32_t ntiles, int32_t mode, int32_t samples, int32_t *first, uint32_t *table, hipStream_t s);   // first [ntiles + 1]
void launch_pt_batch_primary(const PrimaryArgs &a, const PtBatchSamples &sm, const PtBatchChunk &ch, hipStream_t s);      // a.jitter, a.clear_light, the planes but g_light: unused
void launch_pt_batch_trace(const PathTraceArgs &a, const PtBatchSamples &sm, const PtBatchChunk &ch, hipStream_t s);      // a.rng_seed, the planes, a.out: unused; a.do_accumulate must be 0
void launch_pt_batch_accumulate(const StripDev &st, float4 *plane, const int32_t *first, int32_t ntiles, const PtBatchChunk &ch, hipStream_t s);
void launch_pt_batch_close(const StripDev &st, int4 *tiles, int32_t mode, const int32_t *first, const float4 *snap, float4 *out, int32_t n_after, int32_t ntiles, hipStream_t s);

constexpr int kSummaryShards = 1024, kSummaryStride = 32, kSummaryFinal = kSummaryShards * kSummaryStride;
constexpr int kSummaryHeavy = kSummaryFinal + 8;     // tiles on the heavy list of this pass (splat_heavy_kernel)
// Two-level binning of the photon splat, without contended atomics.  Measured (tools/ub/atomics.hip): returning atomics on
// scattered addresses retire at 27 G/s chip-wide (64-byte requests at the memory side), atomics on ONE 128-byte line at 88 M/s
// (11 ns each, whichever words of the line), lines in parallel.  One atomic per (photon, tile) entry on per-tile cursors cost
// 100 us for the 2 M entries of config #3; one per (workgroup, coarse bucket) cost 1.2 ms on 128 bucket cursors packed into four
// lines and 115 us on cursors with a line each (8 k adds per line: a 90 us chain).  So:
//   splat_bin     : a workgroup (kBinChunks x 256 consecutive records) ranks its entries per BUCKET (a rectangle of
//                   2^bucket_w_log2 x 2^bucket_h_log2 = 128 tiles) in LDS and writes them, sorted by bucket, into a segment of its
//                   own + a table of bucket offsets -- no global atomic.
//   splat_scatter : workgroup (slice, bucket): thread t takes the run of bucket entries of bin-workgroup slice * 256 + t, the
//                   workgroup ranks them per tile in LDS and reserves the tiles' bin slots with ONE atomic per (workgroup,
//                   tile): a tile cursor sees one add per slice.
//   splat_big     : photons whose rectangle is larger than 3x3 tiles (huge radii), and those whose entries did not fit into their group's
//                   segment any more, place their entries one atomic each.
#ifndef EVPLP_BIN_CHUNKS
#define EVPLP_BIN_CHUNKS 1
#endif
// 256-record chunks per workgroup of splat_bin_kernel.  Measured (bin + scatter + big kernels, us, configs #3 / #4):
// 1 chunk 155 / 105, 2 chunks 186 / 134, 4 chunks 182 / 128: short workgroups, four per CU, hide latency best.
constexpr int kBinChunks = EVPLP_BIN_CHUNKS;
constexpr int kBinGroup = 256 * kBinChunks;   // records per workgroup
constexpr int kSegCap = 4 * kBinGroup;        // entries of a workgroup's segment: four per record on AVERAGE.  A photon of the LDS path has a rectangle of up to
                                              // 3x3 tiles (nine entries before the depth cull, 1-2 after it); one that no longer fits goes to big_list
#ifndef EVPLP_SCATTER_G
#define EVPLP_SCATTER_G 2
#endif
constexpr int kScatterG = EVPLP_SCATTER_G;    // bin-groups per thread of splat_scatter_kernel (a slice = 256 * kScatterG groups)
constexpr int kMaxBuckets = 1024;
constexpr int kBucketTilesLog2 = 7;   // tiles per bucket: 16 x 8 ...
constexpr int kMaxBucketTilesLog2 = 9; // ... up to 32 x 16 for images of more than 131 072 tiles (kMaxBuckets buckets at most)
struct SplatArgs {
    StripDev st; CamBasis cam;
    evplp_frame_params fp;
    const float4 *g_pos, *g_nrm, *g_dif, *g_phg;
    const evplp_record *records; uint32_t num_records;
    float4 *out;
    // binning workspace: every 8x8-px tile owns a fixed slab of bin_stride item slots
    uint32_t *tile_pairs;     // [ntiles] (photon, pixel) pairs accepted in the tile (statistics; summed by the host on demand)
    float4 *tile_box;         // [ntiles][2] world-space box (lo, hi) of the tile's G-buffer positions
    uint32_t *tile_cursor;    // [ntiles] entries the photons wanted to put into the tile's bin (may exceed bin_stride: overflow)
    uint32_t *bin_items;      // [ntiles][bin_stride] compact photon ids
    uint32_t bin_stride;
    uint32_t *seg;            // [num_bin_groups][kSegCap] entries: record - group base (10 bits) | tile within the bucket (<= 9 bits) << 10, sorted by bucket
    uint16_t *seg_off;        // [num_bin_groups][num_buckets + 1] first entry of every bucket in the group's segment
    uint32_t *big_list;       // [num_bin_groups][kBinGroup] records whose rectangle is larger than 3x3 tiles, and those that overflowed the group's segment
    uint32_t *big_count;      // [num_bin_groups]
    int32_t num_bin_groups, bucket_w_log2, bucket_h_log2, buckets_x, num_buckets;
    uint32_t *bin_items_tmp;  // [ntiles][bin_stride] (deterministic mode: unsorted fill target)
    float4 *compact;          // [num_records * kCompactF4] per-photon pre-shaded data
    uint32_t *overflow;       // device flag: the slots the fullest bin wanted, when that is more than bin_stride (tiles kernel then does nothing; the host re-runs) (fill / tiles then do nothing; the host re-runs)
    uint32_t *summary;        // device: kSummaryShards x {entries, fullest bin} on separate 128-byte lines (scatter / big kernels, per workgroup),
                              // folded into [kSummaryFinal + 0] total bin entries, [+1] entries of the fullest bin by the tile kernel
    int32_t tiles_x, tiles_y; int32_t deterministic; int32_t boxes_valid;   // boxes_valid: tile_box was written by the primary pass
    PassCounters *counters;
    // EVPLP_FOOTPRINT_PROXY (ProxyDev below): the slabs of the proxy mesh in units of the radius, and the per-tile fragment counts
    const float4 *proxy_slabs; const float *proxy_hm; int32_t proxy_count; float proxy_rin, proxy_rout;
    uint32_t *tile_frags;     // [ntiles] proxy fragments accepted in the tile (statistics, like tile_pairs)
    // MIXED tile launches (kernels_splat.hip splat_heavy_kernel): tiles with >= heavy_threshold bin entries, at most heavy_cap of them; null = the pure variants
    uint32_t *heavy_list; uint8_t *tile_flags; uint32_t heavy_cap, heavy_threshold;
};
// The proxy mesh of the reference's photon splat as the tile kernel wants it.  A convex mesh is the intersection of its face planes
// n . x <= h; two faces with opposite normals form a SLAB -h- <= n . x <= h+, and a ray's parameters at the two planes of a slab
// come from one pair of dot products and one reciprocal.  slab i = (n, h+) and hm[i] = h- (kProxyOpen for a face without an opposite
// one).  rin = the smallest h (radius of the largest sphere around the origin inside the mesh), rout = the largest |vertex|.
constexpr int kMaxProxySlabs = EVPLP_MAX_PROXY_PLANES;
constexpr float kProxyOpen = 1.0e15f;
constexpr int kSplatTile = 8;        // pixels per tile edge (one wave per tile)
constexpr int kCompactF4 = 4;        // float4 per compact photon

// dynamic LDS of the kernels that walk the BVH one ray per lane: an [entry][lane] stack as deep as the tree
inline size_t lane_stack_bytes(const SceneDev &sc) { return (size_t)(sc.bvh_depth + 2) * 64 * sizeof(int32_t); }
// (four-wide walk: every second level of the binary tree, up to three pushes per level)
// (four-wide walk: up to three pushes per visit.  3 x levels / 2 is the bound for ANY tree of that depth -- 13 KB per wave for a 31-level
// tree, three waves per SIMD; the bound for THE tree that was built, computed once by evplp_build_accel, is about half of it)
inline size_t lane_stack_bytes4(const SceneDev &sc) {
    const int generic = 3 * ((sc.bvh_depth + 1) / 2) + 4;
    const int entries = sc.stack4_entries > 0 ? (sc.stack4_entries < generic ? sc.stack4_entries : generic) : generic;
    return (size_t)entries * 64 * sizeof(int32_t);
}

void launch_primary(const PrimaryArgs &a, hipStream_t s);
void launch_light_trace(const LightTraceArgs &a, hipStream_t s);
void launch_compact_vpl(const evplp_record *records, uint32_t nrec, evplp_record *out, uint32_t *src_index,
                        uint32_t *count_out, hipStream_t s);
// VPL / VSL gather = the items, then one reduce
void launch_gather_vpl_items(const GatherArgs &a, hipStream_t s, const AdaptArgs &ad = AdaptArgs{});
void launch_gather_vsl(const GatherArgs &a, hipStream_t s, const AdaptArgs &ad = AdaptArgs{});        // walks, then estimators, of the launch's group range
int gather_launch_tiles(const GatherArgs &a);                      // tiles a gather launch enumerates (whole blocks)
void launch_gather_reduce(const GatherArgs &a, int stencil_test, hipStream_t s, const AdaptArgs &ad = AdaptArgs{});
void launch_gather_lvc(const GatherArgs &a, const evplp_record *records, hipStream_t s);
void launch_path_trace(const PathTraceArgs &a, hipStream_t s, const AdaptArgs &ad = AdaptArgs{});     // ad.tiles set: evplp_adaptive_enable_pt's variant
// binning (tile depth ranges, compact photons + bin fill, summary); then the per-tile accumulation
void launch_splat_bin(const SplatArgs &a, hipStream_t s);
void launch_splat_tiles(const SplatArgs &a, bool split_tiles, hipStream_t s, hipEvent_t dominant_begin, hipEvent_t dominant_end);
void launch_resolve(const StripDev &st, const float4 *vpl, const float4 *pm, const float4 *light,
                    float vs, float ps, float ls, int mask_emitter, int gamma, float *out_rgb, hipStream_t s);
// channels: floats per pixel of the gathered strips and of the frame (3: composites; kDenoiseFloats: evplp_group_denoise's packed pixels)
void launch_assemble_strips(const StripDev &st, int nranks, const uint32_t *owner, int chunk_rows, const float *gathered, float *frame, hipStream_t s, int channels = 3);
// EVPLP_PARTITION_ITERATIONS: out = the n planes summed in rank order (fp32, every add rounded), or the first non-zero pixel in rank order
struct ShardPlanes { const float4 *p[64]; };
void launch_reduce_shards(const ShardPlanes &src, int n, int first_nonzero, size_t count, float4 *out, int num_cus, hipStream_t s);
void launch_fill_zero(void *p, size_t bytes, hipStream_t s);
// evplp_frame_error: one image row's figures against the reference (frame_error_kernel, kernels_stats.hip); kept = pixels the mask keeps
struct RowError { double num, rel, rel_kept, kept; };
static_assert(sizeof(RowError) == 32, "RowError must be 32 bytes");
// rgb: the composite (local rows, y = 0 at the bottom); ref: [H][W][3] and keep: [H][W] (null = every pixel), both rows top to bottom;
// rows: [local_rows], zeros for a local row outside the image
void launch_frame_error(const StripDev &st, const float *rgb, const float *ref, const uint8_t *keep, RowError *rows, hipStream_t s);
// evplp_noise_track's planes of one context, one allocation: Q [3][stride] fp64 (one plane per channel; stride = the accumulator plane's
// pixels rounded up to even), then c_prev and c_start [plane pixels] float4 (w = 0).  56 B per pixel.
struct NoisePlanes { double *q; float4 *prev, *start; size_t stride; };
// the moments an estimate reads: one context's (s = null: S = c_prev - c_start, per channel in fp32) or the shards' pooled ones (q and s
// [3][stride] fp64, summed in rank order)
struct NoiseMoments { const double *q, *s; const float4 *prev, *start; size_t stride; };
// out q / s [3][stride]: first ? src : out + src (one shard of the pooling, every add rounded)
void launch_noise_pool(const NoiseMoments &src, bool first, double *q, double *s_out, size_t n, hipStream_t s);
// evplp_adaptive_*: one record per 8 x 8 tile of a context's planes, tile (tx, ty) of local rows 8 ty .. 8 ty + 7 at ty * tiles_x + tx:
// int4 { n_t (0: active; the N at retirement), K_t, B_t (the noise tracker's K and B at retirement), 0 }.  tiles = null: adaptivity is off
// and the noise kernels take their default paths.  n = N, scale: the composite's, both for the retired pixels' frozen variance.
struct AdaptTiles { const int4 *tiles; int32_t tiles_x, pad; double n, scale; };
// the noise launchers (at.tiles == null: the plain kernels; otherwise the variants with retired tiles): the fold leaves a retired pixel's Q
// and c_prev as they are (k = 0 starts tracking whatever at says); the figures and the variance image take a retired pixel's variance as
// noise_var(Q, S, K_t, B_t - 1, (scale N / n_t)^2 K_t)
// fold, k = 0: c_prev = c_start = c, Q = 0 (tracking starts); k >= 1: a batch of k iterations closes (noise_fold_kernel, kernels_stats.hip)
void launch_noise_fold(const NoisePlanes &m, const float4 *vpl, const float4 *pm, const StripDev &st, const AdaptTiles &at, int32_t k, hipStream_t s);
// Non-finite sums (include/evplp.h evplp_noise_track): a pixel is broken when its den or any of its three v = (Q - S^2 / K) / (B - 1) is
// not finite (an emitter pixel under mask_emitter reads no moments: its den alone).  The rows take a broken pixel's num and rel as NaN --
// a report says that it is broken; the tile kernels (adaptive_retire, tile_noise) add nothing for it and do not count it -- a decision
// works around the break; the variance image keeps its bytes (a NaN v reads 0, beyond fp32 reads Inf).
// rows, per local row: { sum num, sum rel, sum rel over kept pixels, kept pixels } of the variance against the composite rgb (layout as frame_error)
void launch_noise_rows(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, const float4 *light, float ls, int mask_emitter,
                       const float *rgb, const uint8_t *keep, RowError *rows, const AdaptTiles &at, hipStream_t s);
// the variance of every plane pixel, 3 floats each (resolve's layout)
void launch_noise_variance(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, float *out_rgb, const AdaptTiles &at, hipStream_t s);
// evplp_adaptive_retire: every active tile whose mean relative variance over its sound in-image pixels (noise_rows_kernel's rel, fp64, summed
// in a fixed tree over the tile's 64 lanes) is <= tau gets the record { n, K, B, 0 } and the snapshot snap = vpl of its pixels; a tile
// without a sound pixel stays active
void launch_adaptive_retire(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, const float4 *light, float ls, int mask_emitter,
                            const float *rgb, double tau, int4 *tiles, int32_t tiles_x, int32_t tiles_y, int32_t n, const float4 *vpl, float4 *snap, hipStream_t s);

// evplp_noise_fold in budget mode, one wavefront per tile with k_t = n_t - K_t: k_t == 0 leaves the tile alone; otherwise per pixel and channel
// D = R - c_prev (fp32), Q += D * D / k_t (fp64, noise_fold_kernel's order), c_prev = R, then lane 0 writes K_t = n_t, B_t += 1
void launch_noise_fold_budget(const NoisePlanes &m, const StripDev &st, int4 *tiles, const float4 *snap, int32_t ntiles, hipStream_t s);
// evplp_adaptive_tile_noise: out[tile] = the mean of rel over the tile's sound in-image pixels as adaptive_retire_kernel forms it (0: no such pixel)
void launch_tile_noise(const StripDev &st, const NoiseMoments &m, double K, double B, double s2K, const float4 *light, float ls, int mask_emitter,
                       const float *rgb, const AdaptTiles &at, int32_t ntiles, double *out, hipStream_t s);

// evplp_denoise (kernels_denoise.hip): one pixel as the a-trous passes read it.  u = (c / albedo, luminance variance s) of a filtered pixel,
// (composite, 0) of any other; pos.w = 1 for a filtered pixel, 0 otherwise; albedo = max(diffuse + phong, 1e-3); rgb = the composite.
// 80 B, 20 floats: the strips of a group are exchanged and assembled as floats (assemble_strips_kernel, kDenoiseFloats channels).
struct DenoisePixel { float4 u, pos, nrm, albedo, rgb; };
static_assert(sizeof(DenoisePixel) == 80, "DenoisePixel must be 80 bytes");
constexpr int kDenoiseFloats = (int)(sizeof(DenoisePixel) / sizeof(float));
// the packed pixels of a context's planes (local rows): rgb = the composite, var = the noise tracker's variance, 3 floats per pixel each;
// out: [W * local_rows] DenoisePixel
void launch_denoise_prepare(const StripDev &st, const float *rgb, const float *var, const float4 *pos, const float4 *nrm, const float4 *dif,
                            const float4 *phg, const float4 *light, float4 *out, hipStream_t s);
// one a-trous pass over a frame of W x rows packed pixels (rows from the bottom); in: (u, s) every in_step float4, out: a plane of (u', s')
struct DenoiseLevelArgs {
    const DenoisePixel *frame; const float4 *in; float4 *out;
    int32_t W, rows, in_step, h;
    float sigma_l, sigma_n, sigma_x_r, pad;      // sigma_x_r = sigma_position * the bounding-sphere radius
};
void launch_denoise_level(const DenoiseLevelArgs &a, hipStream_t s);
// out_rgb [n][3]: albedo * u of a filtered pixel, the composite of any other
void launch_denoise_finish(const DenoisePixel *frame, const float4 *u, size_t n, float *out_rgb, hipStream_t s);

// evplp_denoise_temporal (kernels_temporal.hip).  prev_pose_kernel walks like primary_kernel (same arguments, the jitter and light flags of
// the pass that wrote the G-buffer in memory) and evaluates every pixel's hit (tri, b, g) on prev_v, 9 floats per original triangle: the
// pose at the end of the previous call.  pos = (P_prev, tri >= 0 ? 1 : 0), nrm = (N_prev, 0); 32 B per plane pixel, exchanged and assembled
// as floats like the packed pixels.  debug (tests; null otherwise): (bits of tri, b, g, 0).  prev null: the debug plane alone.
struct TemporalPrev { float4 pos, nrm; };
constexpr int kTemporalPrevFloats = (int)(sizeof(TemporalPrev) / sizeof(float));
void launch_prev_pose(const PrimaryArgs &a, const float *prev_v, TemporalPrev *prev, float4 *debug, hipStream_t s);
// prev_v[9 t + k] = attrs[t].v[k]
void launch_pose_snapshot(const TriAttr *attrs, int32_t ntri, float *prev_v, hipStream_t s);
// The accumulation stage over a frame of W x rows packed pixels (rows from the bottom, image rows 0 .. H - 1): writes (u_out, s_out) into
// frame[i].u and the new history.  A history is three planes of `px` float4: (u, s), (X, filtered), (n, length).  has_history = 0: every
// filtered pixel starts a history.  counts: { filtered, reprojected, disoccluded, summed history length } of every workgroup of 16 x 16
// pixels, [temporal_count_slots(W, rows)]; the host adds the slots.
int temporal_count_slots(int W, int rows);
struct TemporalArgs {
    DenoisePixel *frame; const TemporalPrev *prev; const float4 *h_in; float4 *h_out; uint4 *counts;
    size_t px;
    int32_t W, rows, H, has_history;
    CamBasis cam, prev_cam;
    float sigma_x_r, normal_cos, max_history, pad;
};
void launch_temporal_accumulate(const TemporalArgs &a, hipStream_t s);

} // namespace evplp
