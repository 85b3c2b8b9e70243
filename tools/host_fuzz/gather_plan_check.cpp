// The gathers' launch plan (csrc/host/gather_plan.cpp) without a GPU, for tests/test_gather_plan_host.py, which builds this with
// AddressSanitizer + UndefinedBehaviorSanitizer: hand-derived known answers, then the plan's invariants over a seeded sweep of frames, strips,
// slot counts, overrides and bounds -- bands and group ranges tile the frame and the groups exactly once, within the bounds they were cut for.
#include "gather_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace evplp;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n  W %d rows %d/%d strips %d x %d slots %zu vsl %d k %d/%d deal %d block %d cuts %d/%d caps %zu %zu\n", __LINE__, #cond, \
    in.W, in.local_rows, in.rows_in_image, in.strip_count, in.strip_rows, in.nvpl_slots, (int)in.vsl, in.splits_per_wave, in.env_gather_k, in.env_item_deal, in.env_tile_block_log2, \
    in.env_cuts, (int)in.cuts_available, in.cut_cap, in.mask_cap); std::exit(1); } } while (0)

static const size_t GiB = (size_t)1 << 30;

// one context of one strip (evplp_create: the strip is the image's rows rounded up to whole tiles), nothing overridden, the default bounds
static GatherPlanInput single(int W, int H, size_t slots, bool vsl) {
    GatherPlanInput in{};
    in.W = W; in.local_rows = in.strip_rows = (H + 7) / 8 * 8; in.rows_in_image = H; in.strip_count = 1;
    in.nvpl_slots = slots; in.vsl = vsl;
    in.env_item_deal = in.env_tile_block_log2 = in.env_cuts = -1;
    in.cut_cap = 8 * GiB; in.mask_cap = 2 * GiB; in.cuts_available = true;
    return in;
}

struct Seen { long plans = 0, refused = 0, banded = 0, ranged = 0, both = 0, no_cuts = 0; };

// the invariants of one plan; what it was planned for comes along for the message
static void check_plan(const GatherPlanInput &in, Seen &seen) {
    const GatherPlan p = plan_gather(in);
    // the refusal: a VSL gather whose items hold more than 4095 VSLs even at k = 1 -- and nothing else
    const bool must_refuse = in.vsl && in.nvpl_slots / 128 + 1 > 4095;
    CHECK((p.refused != nullptr) == must_refuse);
    if (p.refused) { seen.refused++; return; }
    seen.plans++;
    // k: a power of two in 1 .. 32 within both counter limits; the precedence of its sources where no limit halves it
    const size_t per_split = in.nvpl_slots / 128 + 1;
    CHECK(p.k >= 1 && p.k <= 32 && (p.k & (p.k - 1)) == 0 && p.groups * p.k == 128);
    CHECK(p.k == 1 || per_split * (size_t)p.k < 65536);
    CHECK(!in.vsl || per_split * (size_t)p.k <= 4095);
    const bool small_launch = (size_t)((in.W + 7) / 8) * (size_t)((in.rows_in_image + 7) / 8) <= 8192;
    const int asked = in.env_gather_k > 0 ? in.env_gather_k : in.splits_per_wave > 0 ? in.splits_per_wave : small_launch ? 1 : 2;
    CHECK(p.k <= asked && (p.k == asked || per_split * (size_t)(2 * p.k) >= 65536 || (in.vsl && per_split * (size_t)(2 * p.k) > 4095)));
    CHECK(p.item_deal == (in.env_item_deal >= 0 ? in.env_item_deal : small_launch ? 1 : 0));
    // tile blocks: a power of two of tile rows, at most 8, that a strip keeps adjacent
    const int sh = 1 << p.block_h_log2;
    CHECK(p.block_h_log2 >= 0 && p.block_h_log2 <= 3 && (in.env_tile_block_log2 < 0 || p.block_h_log2 <= in.env_tile_block_log2));
    CHECK(in.strip_count == 1 || (in.strip_rows / 8) % sh == 0);
    CHECK(p.tiles_y == (in.local_rows + 7) / 8 && p.nby == (p.tiles_y + sh - 1) / sh);
    // fallbacks: no cuts asked for, none to be had, or a bound below one row of tile blocks -> one band from the root
    if (in.env_cuts == 0 || !in.cuts_available) CHECK(!p.use_cuts);
    if (!p.use_cuts) { CHECK(p.nbands == 1 && p.band_rows == p.nby && p.cut_bytes == 0); seen.no_cuts++; }
    size_t row_bytes = 0;
    if (p.use_cuts) {
        const bool neighbours = in.strip_count == 1 || in.strip_rows >= 16;
        CHECK(p.gw_log2 == 1 && p.gh_log2 == ((sh >= 2 && neighbours) ? 1 : 0) && p.groups_x == ((in.W + 7) / 8 + 1) / 2 && p.vpl_stride == (uint32_t)in.nvpl_slots);
        row_bytes = (size_t)p.groups_x * p.vpl_stride * 256;                     // one row of tile groups
        CHECK(p.cut_bytes <= in.cut_cap && p.cut_bytes == (size_t)p.band_rows * (sh >> p.gh_log2) * row_bytes);
        // (as many rows as the bound holds: one more would not fit, or there is no more)
        CHECK(p.band_rows == p.nby || (size_t)(p.band_rows + 1) * (sh >> p.gh_log2) * row_bytes > in.cut_cap);
    } else if (in.env_cuts != 0 && in.cuts_available)
        CHECK((size_t)(sh >> ((sh >= 2 && (in.strip_count == 1 || in.strip_rows >= 16)) ? 1 : 0)) * (((in.W + 7) / 8 + 1) / 2) * (uint32_t)in.nvpl_slots * 256 > in.cut_cap || (uint32_t)in.nvpl_slots == 0);
    // bands tile [0, nby) once and in order; their group rows follow on from one another and end with the frame's last
    CHECK(p.nbands >= 1 && p.band_rows >= 1);
    int next_row = 0, next_group_row = 0;
    const size_t per_item = (size_t)p.k * (size_t)p.masks_per_split * 8;
    for (int i = 0; i < p.nbands; i++) {
        const GatherBand b = gather_band(p, i);
        CHECK(b.first == next_row && b.rows >= 1 && b.rows <= p.band_rows && b.args_rows == (p.nbands > 1 ? b.rows : 0));
        next_row += b.rows;
        if (p.use_cuts) {
            CHECK(b.group_row_first == next_group_row && b.groups_y >= 1 && (size_t)b.groups_y * row_bytes <= p.cut_bytes);
            CHECK(b.group_row_first == (b.first * sh) >> p.gh_log2);             // the band's first tile row opens a group row
            next_group_row += b.groups_y;
        }
        // group launches tile [0, 128 / k) once, and no launch of any band needs more masks than the buffer holds
        const size_t tiles = (size_t)gather_band_tiles(in.W, in.local_rows, p.block_h_log2, b.first, b.args_rows);
        CHECK(tiles == (size_t)((in.W + 7) / 8 + 7) / 8 * 8 * (size_t)b.rows * sh);
        int next_group = 0;
        for (int j = 0; j < p.group_launches; j++) {
            const GatherGroupRange r = gather_group_range(p, j);
            CHECK(r.first == next_group && r.count >= 1 && r.count <= p.groups_per_launch);
            CHECK(!in.vsl || tiles * (size_t)r.count * per_item <= p.mask_bytes);
            next_group += r.count;
        }
        CHECK(next_group == p.groups);
    }
    CHECK(next_row == p.nby);
    if (p.use_cuts) CHECK(next_group_row == (p.tiles_y + (1 << p.gh_log2) - 1) >> p.gh_log2);
    if (in.vsl) {
        CHECK(p.masks_per_split == (int32_t)((in.nvpl_slots + 127) / 128) && p.mask_bytes > 0);
        CHECK(p.mask_bytes <= in.mask_cap || p.groups_per_launch == 1);
    } else CHECK(p.masks_per_split == 0 && p.mask_bytes == 0 && p.group_launches == 1 && p.groups_per_launch == p.groups);
    seen.banded += p.nbands > 1; seen.ranged += p.group_launches > 1; seen.both += p.nbands > 1 && p.group_launches > 1;
}

int main() {
    Seen seen;
    {   // 1024 x 1024, 4096 slots (config #2 / #3): one band of 4 GiB -- the documented 4.3 GB --, 512 MiB of masks in one launch
        GatherPlanInput in = single(1024, 1024, 4096, true);
        const GatherPlan p = plan_gather(in);
        CHECK(!p.refused && p.k == 2 && p.groups == 64 && p.item_deal == 0 && p.block_h_log2 == 3 && p.nby == 16);
        CHECK(p.use_cuts && p.gw_log2 == 1 && p.gh_log2 == 1 && p.groups_x == 64 && p.vpl_stride == 4096);
        CHECK(p.nbands == 1 && p.band_rows == 16 && p.cut_bytes == 16 * (size_t)268435456 && p.cut_bytes == (size_t)4294967296);
        CHECK(p.masks_per_split == 32 && p.mask_bytes == 512 << 20 && p.group_launches == 1 && p.groups_per_launch == 64);
        CHECK(gather_band(p, 0).args_rows == 0 && gather_band(p, 0).groups_y == 64);
        in.vsl = false; CHECK(plan_gather(in).k == 2 && plan_gather(in).cut_bytes == p.cut_bytes && plan_gather(in).mask_bytes == 0);
        in.cuts_available = false; CHECK(!plan_gather(in).use_cuts && plan_gather(in).nbands == 1);
        check_plan(in, seen);
    }
    {   // 2048 x 2048, 16 384 slots: 2 GiB of cut slots per row of tile blocks -> eight bands of four rows, 1 GiB of masks per band
        GatherPlanInput in = single(2048, 2048, 16384, true);
        const GatherPlan p = plan_gather(in);
        CHECK(!p.refused && p.k == 2 && p.item_deal == 0 && p.block_h_log2 == 3 && p.nby == 32 && p.gh_log2 == 1 && p.groups_x == 128);
        CHECK(p.use_cuts && p.band_rows == 4 && p.nbands == 8 && p.cut_bytes == 8 * GiB && p.cut_bytes / 4 == 2 * GiB);
        CHECK(p.masks_per_split == 128 && p.mask_bytes == GiB && p.group_launches == 1);
        CHECK(gather_band(p, 7).first == 28 && gather_band(p, 7).rows == 4 && gather_band(p, 7).args_rows == 4 && gather_band(p, 7).group_row_first == 112 && gather_band(p, 7).groups_y == 16);
        check_plan(in, seen);
    }
    {   // 96 x 192 on one context: a small launch -- short items dealt over all XCDs
        GatherPlanInput in = single(96, 192, 384, false);
        const GatherPlan p = plan_gather(in);
        CHECK(p.k == 1 && p.groups == 128 && p.item_deal == 1 && p.block_h_log2 == 3 && p.nby == 3 && p.nbands == 1 && p.gh_log2 == 1);
        CHECK(p.use_cuts && p.cut_bytes == 3 * (size_t)2359296);
        // (EVPLP_CUT_BYTES=1000000 of tests/test_gpu_parity.py test_entry_cuts_do_not_change_a_bit is below ONE row of tile blocks here: that
        // case walks from the root in one band; three bands take a bound of 2 359 296 .. 4 718 591 bytes)
        in.cut_cap = 1000000; CHECK(!plan_gather(in).use_cuts && plan_gather(in).nbands == 1);
        in.cut_cap = 2359296; CHECK(plan_gather(in).use_cuts && plan_gather(in).nbands == 3);
        check_plan(in, seen);
    }
    for (int strip_rows : { 8, 16 }) {      // strips of 8 rows: single tile rows, 2 x 1 groups; of 16 rows: blocks of two tile rows, 2 x 2 groups
        GatherPlanInput in = single(256, 256, 1024, true);
        in.strip_count = 4; in.strip_rows = strip_rows; in.local_rows = 64; in.rows_in_image = 64;
        const GatherPlan p = plan_gather(in);
        CHECK(p.block_h_log2 == (strip_rows == 8 ? 0 : 1) && p.use_cuts && p.gh_log2 == (strip_rows == 8 ? 0 : 1) && p.nby == (strip_rows == 8 ? 8 : 4));
        check_plan(in, seen);
    }
    {   // the frame of tests/test_gpu_parity.py test_gather_bands_and_group_ranges_do_not_change_a_bit with its two byte overrides: 9 x 17
        // tiles (ragged block columns, a ragged last block row), 64 paths x 4 photons
        GatherPlanInput in = single(72, 136, 256, true);
        in.cut_cap = 2000000; in.mask_cap = 50000;
        GatherPlan p = plan_gather(in);
        CHECK(p.k == 1 && p.nby == 3 && p.use_cuts && p.nbands >= 3 && p.group_launches >= 4);
        CHECK(p.nbands == 3 && p.groups_per_launch == 16 && p.group_launches == 8 && p.mask_bytes == 32768 && p.cut_bytes == 1310720);
        CHECK(gather_band(p, 2).groups_y == 1 && gather_band(p, 2).group_row_first == 8);       // (17 tile rows: nine group rows, the last of one tile row)
        check_plan(in, seen);
        in.vsl = false; CHECK(plan_gather(in).nbands == 3); check_plan(in, seen);
        in.vsl = true; in.cut_cap = 8 * GiB;                                                    // EVPLP_MASK_BYTES alone: one band, sixteen launches
        p = plan_gather(in);
        CHECK(p.nbands == 1 && p.groups_per_launch == 8 && p.group_launches == 16 && p.mask_bytes == 384 * 8 * 16);
        check_plan(in, seen);
    }
    {   // the VSL limit: 4094 * 128 slots are gathered (at k = 1), one more is refused; the VPL gather takes them at k <= 8
        GatherPlanInput in = single(64, 64, 4094 * 128 + 127, true);
        CHECK(!plan_gather(in).refused && plan_gather(in).k == 1);
        in.nvpl_slots++; CHECK(plan_gather(in).refused);
        in.vsl = false; in.env_gather_k = 32; CHECK(!plan_gather(in).refused && plan_gather(in).k == 8);
    }
    // the sweep
    std::mt19937_64 rng(20240611);
    auto pick = [&](size_t n) { return (size_t)(rng() % n); };
    auto log_uniform = [&](int bits) { const int b = (int)pick((size_t)bits + 1); return (((size_t)1 << b) | (rng() & (((size_t)1 << b) - 1))); };
    static const int kLarge[][2] = { { 1024, 1024 }, { 2048, 2048 }, { 4096, 2048 }, { 1920, 1080 }, { 8192, 8192 } };
    static const size_t kSlots[] = { 1, 127, 128, 129, 4094, 4095 * 128 - 1, 4094 * 128 + 127, 4095 * 128, 4095 * 128 + 1, 511 * 128, 512 * 128, 65535 * 128, 65536 * 128, 8388608 };
    for (int it = 0; it < 400000; it++) {
        GatherPlanInput in{};
        int H;
        if (pick(16) == 0) { const int *wh = kLarge[pick(5)]; in.W = wh[0]; H = wh[1]; } else { in.W = 1 + (int)pick(300); H = 1 + (int)pick(300); }
        if (pick(2)) { in.strip_count = 1; in.strip_rows = in.local_rows = (H + 7) / 8 * 8; in.rows_in_image = H; }
        else {      // evplp_create's arithmetic of a strip partition; any number of the strip's rows may lie inside the image
            in.strip_count = 2 + (int)pick(7); in.strip_rows = 8 << pick(3);
            const int nblocks = (H + in.strip_rows - 1) / in.strip_rows, owned = (nblocks + in.strip_count - 1) / in.strip_count;
            in.local_rows = owned * in.strip_rows; in.rows_in_image = (int)pick((size_t)in.local_rows + 1);
        }
        switch (pick(4)) {
        case 0: in.nvpl_slots = kSlots[pick(sizeof(kSlots) / sizeof(kSlots[0]))]; break;
        case 1: in.nvpl_slots = 1 + pick(2048); break;
        default: in.nvpl_slots = log_uniform(23); break;
        }
        in.vsl = pick(2) != 0;
        in.splits_per_wave = pick(2) ? 0 : 1 << pick(6);
        in.env_gather_k = pick(3) ? 0 : 1 << pick(6);
        in.env_item_deal = (int)pick(3) - 1; in.env_tile_block_log2 = pick(2) ? -1 : (int)pick(5); in.env_cuts = (int)pick(3) - 1;
        in.cut_cap = pick(4) ? log_uniform(40) : 8 * GiB; in.mask_cap = pick(4) ? log_uniform(40) : 2 * GiB;
        if (pick(64) == 0) in.cut_cap = 1;
        if (pick(64) == 0) in.mask_cap = 1;
        in.cuts_available = pick(8) != 0;
        check_plan(in, seen);
    }
    std::printf("plans %ld refused %ld banded %ld ranged %ld both %ld rootwalks %ld\n", seen.plans, seen.refused, seen.banded, seen.ranged, seen.both, seen.no_cuts);
    return 0;
}
