"""The statistics kernels (kernels_stats.hip) on the hostile sums of tests/stats_hostile.py, against the shared numpy restatement (the
variance image's bytes, figures to 1e-12) and against the independent float64 statement (the derived bar): one context with the plain and
with the tile-record instantiations of the kernels, the per-tile figures of evplp_adaptive_tile_noise, evplp_frame_error against hostile
references, two row strips, the iteration partition's pooled moments, retirement on a path-traced and on a gathered room with poisoned accumulators, and
both budget modes.

Measured on one MI355X, 2026-10-21 (the whole file: 70 tests in 3.5 s).  Worst error / bar of the kernels against statement64, per family:
  family          variance   figures   tile figures   pooled variance / figures (iteration partition)
  decades         0.699      0.0191    0.0586         0.699 / 0.0191
  late_start      0.625      2.0e-10   1.9e-10        0.625 / 1.9e-10
  inexact_S       0.0937     0.0184    0.0255         0.0937 / 0.0184
  zero_variance   0.0933     0.0198    0.0247         0.0933 / 0.0157
  emitters        0.171      0.00316   0.0295         -
  nonfinite       0.688      0 (NaN by NaN)  0.1      0.688 / 0
  masks           0.692      0.1       0.1            -
(the plain and the tile-record instantiations give the same doubles, and both equal the restatement: bytes, 1e-12).  Retirement: tile
figures 0.0136 of the bar (pt) and 0.0057 (gather), at retirement and frozen; tau in a gap of 1.8e5 and 3.1e4 bars; the tile with one Inf
pixel reads the mean of its 63 sound pixels (pt 0.0480086, gather 0.0178903, statement64 the same digits).  Budget modes, per budget
0 / 1 / 2: pt tiles 0.0097 / 0.0109 / 0.017, variance 0.28 / 0.25 / 0.26; gather tiles 0.0022 / 0.0060 / 0.0013, variance 0.17 / 0.20 / 0.16.

On the parent commit's kernels_stats.hip (the same library otherwise) 24 of the 70 fail, the other 46 pass:
  - test_one_context_against_both_references, 18: every nonfinite, masks and emitters case, both instantiations.  The Inf pixel reads as
    converged -- the figures are finite or Inf where the rule says NaN (nonfinite-5x3: (6.25e38, 0.01067, 0.01067), the relative figures
    silently smaller) -- and with the tile records the tile figures hold NaN, which evplp_plan_budgets refuses (8 of the 18 end there).
  - test_the_iteration_partition_pools_to_the_pooled_statement, 2: the nonfinite cases, the same figures through the pool.
  - test_retirement_judges_a_tile_by_its_sound_pixels, 2 (pt, gather): the all-broken tile's figure is NaN, not 0.
  - test_pt_budget_mode_.. and test_gather_budget_mode_.., 1 each: NaN tile figures, the planner refuses the plan.
The finite families, evplp_frame_error and the two strips pass on both: no bit changed on finite inputs.

Not here: the technique loops' "noise" block with a NaN figure.  evplp_render_json owns its context and offers no hook to poison a sum; by
its code (technique.cpp, class Noise: num() and the stopRelMse comparison) a non-finite figure is written as null, which json.load reads, and NaN <= stopRelMse
is false, so it does not stop the run."""
from types import SimpleNamespace

import numpy as np
import pytest

import scenes
import stats_hostile as sh
from stats_hostile import f32, f64
from test_gpu_convergence import numpy_error

pytestmark = pytest.mark.gpu

CASES = sh.CASES
WORST = {}


def note(what, family, ratio):
    key = (what, family)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{what}, {family}: worst error / bar so far {WORST[key]:.3g}")


def same_figures(got, want):
    return all(sh.figure_ratio(g, w, 0.0) == 0.0 for g, w in zip(got, want))


def check_call(case, e, light, what, tiles=None):
    """one estimate of the device against both references; returns the references"""
    rs = sh.restate(case, e.scale, e.ls, e.me, e.composite, light)
    ref = sh.statement64(case, e.scale, e.ls, e.me, e.composite, light)
    tag = (sh.case_id((case.family, case.W, case.H, case.variant)), e.scale, e.ls, e.me)
    assert sh.same_nan(e.var, sh.to32(rs.var)), tag                                      # the variance image: bytes
    assert sh.worst_ratio(e.figs, rs.figs, [1e-12 * abs(f) + 1e-300 for f in rs.figs]) <= 1.0, (tag, e.figs, rs.figs)
    assert [bool(np.isnan(f)) for f in e.figs] == [bool(np.isnan(f)) for f in ref.figs], (tag, e.figs, ref.figs)   # NaN exactly where the rule says
    rv, rf = sh.variance_ratio(e.var, ref), sh.worst_ratio(e.figs, ref.figs, ref.fig_bars)
    note(what + " variance", case.family, rv); note(what + " figures", case.family, rf)
    assert rv <= 1.0 and rf <= 1.0, (tag, rv, rf, e.figs, ref.figs, ref.fig_bars)
    if tiles is not None:
        assert np.isfinite(tiles).all() and (tiles >= 0).all(), tag
        assert sh.worst_ratio(tiles, rs.tiles, 1e-12 * np.abs(rs.tiles) + 1e-300) <= 1.0, (tag, tiles, rs.tiles)
        rt = sh.worst_ratio(tiles, ref.tiles, ref.tile_bars)
        note(what + " tiles", case.family, rt)
        assert rt <= 1.0, (tag, rt)
        empty = sh.broken_per_tile(ref.broken) == sh.in_image_per_tile(case.W, case.H)
        assert (tiles[empty] == 0.0).all()                                               # no sound pixel: the tile reads 0
    return rs, ref


_single = {}


def single(evplp, key, adaptive=False):
    """the case on one context: its estimates (and, with the tile records allocated, its tile figures), computed once per key"""
    if (key, adaptive) not in _single:
        case = sh.make_case(*key)
        with evplp.Context(case.W, case.H, 1, 1, 1) as c:
            assert c.local_rows == case.rows
            if adaptive:            # (before the folds: every fold and every estimate then runs the kernels' tile-record instantiation)
                c.upload(evplp.BUF_VPL_ACCUM, case.states[0]); c.noise_track(True); c.adaptive_enable(True)
            sh.upload_case(evplp, c, case)
            est = sh.estimates(c, case)
            light = c.download(evplp.BUF_LIGHT)[:case.H]
            tiles = [c.adaptive_tile_noise(s, ls, mask_emitter=me) for s, ls, me in case.calls] if adaptive else [None] * len(est)
            plan = None
            if adaptive:
                plan = evplp.plan_budgets(tiles[0], np.full(tiles[0].shape, case.K, np.int32), 16, 1, 0.0, 1.0)
        _single[(key, adaptive)] = SimpleNamespace(case=case, est=est, light=light, tiles=tiles, plan=plan)
    return _single[(key, adaptive)]


@pytest.mark.parametrize("adaptive", [False, True], ids=["plain", "records"])
@pytest.mark.parametrize("key", CASES, ids=sh.case_id)
def test_one_context_against_both_references(evplp, key, adaptive):
    r = single(evplp, key, adaptive)
    case = r.case
    assert r.light.tobytes() == case.light[:case.H].tobytes()
    for e, t in zip(r.est, r.tiles):
        check_call(case, e, r.light, "records" if adaptive else "plain", t)
    if adaptive:
        assert r.plan.size == r.tiles[0].size and (r.plan >= 1).all()      # the planner takes the figures, a NaN pixel in the frame or not
        plain = single(evplp, key, False)
        for a, b in zip(r.est, plain.est):
            assert same_figures(a.figs, b.figs) and sh.same_nan(a.var, b.var)            # both instantiations: the same doubles


@pytest.mark.parametrize("W, H", sh.FRAMES)
def test_frame_error_propagates_what_is_not_finite(evplp, W, H):
    """evplp_frame_error's terms are fp32 in the reference's order; a non-finite term makes the figures it enters non-finite"""
    seen = set()
    for fam in ("zero_variance", "nonfinite"):
        case = sh.make_case(fam, W, H)
        s = 1.0 / case.K
        with evplp.Context(W, H, 1, 1, 1) as c:
            for b, p in ((evplp.BUF_LIGHT, case.light), (evplp.BUF_PHOTON_ACCUM, case.photon), (evplp.BUF_VPL_ACCUM, case.states[-1])):
                c.upload(b, p)
            for name, ref, mask in sh.error_references(W, H):
                c.set_error_reference(ref, mask)
                for scale, gamma in ((s, False), (s, True), (-s, True), (1e20, False)):
                    img = c.resolve(scale, scale, 1.0, gamma=gamma)[:H]
                    got = c.frame_error(scale, scale, 1.0, gamma=gamma)
                    with np.errstate(all="ignore"):
                        want = numpy_error(img, ref, mask)
                    ok = sh.worst_ratio(got, want, [1e-12 * abs(w) + 1e-300 for w in want]) <= 1.0
                    assert ok, (fam, name, scale, gamma, got, want)
                    seen |= {"nan" if np.isnan(w) else "inf" if np.isinf(w) else "finite" for w in want}
                    if fam == "zero_variance" and mask is not None and scale == s and not gamma:
                        assert np.isfinite(want[2]) and not np.isfinite(want[0]), (name, want)      # the mask keeps the hostile pixels out
                    if scale < 0 and gamma:
                        assert np.isnan(img).any() and np.isnan(want[0])                             # powf of a negative composite
    assert seen == {"nan", "inf", "finite"}, seen


def strip_plane(full, local_rows, rank, ranks, H):
    """the rows of a whole-image plane that rank `rank` of `ranks` strips of 8 rows holds (blocks b % ranks == rank, in order); a local row
    past the image is hostile like the image's own rows past H"""
    out = np.empty((local_rows, full.shape[1], 4), f32)
    out[:, 0::2] = f32(1e30); out[:, 1::2] = f32(np.nan)
    for l in range(local_rows):
        y = ((l // 8) * ranks + rank) * 8 + l % 8
        if y < H:
            out[l] = full[y]
    return out


@pytest.mark.parametrize("key", CASES, ids=sh.case_id)
def test_two_row_strips_give_the_same_doubles(evplp, key):
    one = single(evplp, key, False)
    case = one.case
    with evplp.Group(case.W, case.H, 1, 1, 1, 2, devices=[0, 0], strip_rows=8) as g:
        ranks = [g.rank(r) for r in range(2)]

        def upload(which, full):
            for r, c in enumerate(ranks):
                c.upload(which, strip_plane(full, c.local_rows, r, 2, case.H))

        upload(evplp.BUF_LIGHT, case.light); upload(evplp.BUF_PHOTON_ACCUM, case.photon); upload(evplp.BUF_VPL_ACCUM, case.states[0])
        g.noise_track(True, case.mask)
        for k, s in zip(case.schedule, case.states[1:]):
            upload(evplp.BUF_VPL_ACCUM, s)
            g.noise_fold(k)
        for (scale, ls, me), e in zip(case.calls, one.est):
            got = g.noise_estimate(scale, ls, mask_emitter=me)
            assert same_figures(got, e.figs), (scale, ls, me, got, e.figs)
            assert sh.same_nan(g.noise_variance(scale), e.var), (scale, ls, me)


POOLED = [k for k in CASES if k[0] in ("decades", "inexact_S", "zero_variance", "nonfinite", "late_start") and k[1] != 5]


@pytest.mark.parametrize("key", POOLED, ids=sh.case_id)
def test_the_iteration_partition_pools_to_the_pooled_statement(evplp, key):
    """rank 0 tracks the case's first two folds, rank 1 -- on sums of its own that start where rank 0's end -- the last two: noise_pool_kernel
    adds the shards' Q and S, and the pooled batches are the case's four.  The composite is the sum of both ranks' sums."""
    case = sh.make_case(*key)
    H = case.H
    with evplp.Group(case.W, H, 1, 1, 1, 2, devices=[0, 0], partition="iterations") as g:
        for r in range(2):
            c = g.rank(r)
            assert c.local_rows == case.rows
            c.upload(evplp.BUF_LIGHT, case.light); c.upload(evplp.BUF_PHOTON_ACCUM, case.photon)
            c.upload(evplp.BUF_VPL_ACCUM, case.states[2 * r])
        g.noise_track(True, case.mask)
        for r in range(2):
            g.select_rank(r)
            for j in (2 * r + 1, 2 * r + 2):
                g.rank(r).upload(evplp.BUF_VPL_ACCUM, case.states[j])
                g.noise_fold(case.schedule[j - 1])
        sums = [s[:H, :, :3] for s in case.states]
        shards = [(sums[0:3], case.schedule[0:2]), (sums[2:5], case.schedule[2:4])]
        for scale, ls, me in case.calls:
            figs = g.noise_estimate(scale, ls, mask_emitter=me)
            var = g.noise_variance(scale)
            comp = g.resolve(scale, scale, ls, mask_emitter=me)
            ref = sh.statement64(case, scale, ls, me, comp, shards=shards)
            assert [bool(np.isnan(f)) for f in figs] == [bool(np.isnan(f)) for f in ref.figs], (scale, figs, ref.figs)
            rv, rf = sh.variance_ratio(var, ref), sh.worst_ratio(figs, ref.figs, ref.fig_bars)
            note("pooled variance", case.family, rv); note("pooled figures", case.family, rf)
            assert rv <= 1.0 and rf <= 1.0, (scale, ls, me, rv, rf, figs, ref.figs)
            if case.family == "nonfinite":
                assert np.isnan(figs[0]) and not (var < 0).any()                         # the broken pixels come through the pool


# ---- retirement on real accumulating calls: evplp_adaptive_retire returns 0 while N = 0, so the sums come from a path tracer or a gather on a
# small box room, and the accumulator is downloaded, poisoned and uploaded again after the first iteration (a sum keeps what is not finite)
RW, RH = 37, 21
RETIRE_AT = 4
JIT = (0.004, -0.003)
ONE, ALL = (3, 2), (1, 1)             # the pixel of tile (0, 0) that holds +Inf; the tile whose every pixel is broken


def room_iteration(evplp, c, room, mode, i):
    c.primary(JIT)
    if mode == "pt":
        c.path_trace(room.cam_origin, i, 3)
        return
    r = 0.4
    fp = evplp.frame_params(camera_pos=room.cam_origin, mis_mode=1, pdf_mc=1.0 / (np.pi * r * r), photon_radius=r, num_light_paths=32,
                            num_vpl_light_paths=32, photons_per_path=4, do_accumulate=1, rng_seed=i, jitter=JIT)
    c.trace_light_paths(i); c.gather_vpl(fp)


def tracked_case(evplp, c, states, schedule):
    """what stats_hostile's references want of a case, from the planes of a running context"""
    return SimpleNamespace(family="room", W=RW, H=RH, variant=0, rows=c.local_rows, states=list(states), photon=c.download(evplp.BUF_PHOTON_ACCUM),
                           light=c.download(evplp.BUF_LIGHT), mask=None, schedule=tuple(schedule), K=sum(schedule), B=len(schedule))


@pytest.mark.parametrize("mode", ["pt", "gather"])
def test_retirement_judges_a_tile_by_its_sound_pixels(evplp, mode):
    room = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=RW / RH)
    ctx = evplp.Context(RW, RH, 1, 1, 1) if mode == "pt" else evplp.Context(RW, RH, 32, 32, 4, deterministic=True)
    with ctx as c:
        room.upload(c)
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, path_trace=(mode == "pt"))
        states = [c.download(evplp.BUF_VPL_ACCUM)]
        assert not states[0][:RH].any()
        for i in range(RETIRE_AT):
            room_iteration(evplp, c, room, mode, i)
            if i == 0:
                acc = c.download(evplp.BUF_VPL_ACCUM)
                acc[ONE[0], ONE[1], 0] = np.inf
                n = 0
                for y in range(8 * ALL[0], 8 * ALL[0] + 8):
                    for x in range(8 * ALL[1], 8 * ALL[1] + 8):
                        acc[y, x, n % 3] = (np.inf, -np.inf, np.nan)[(n // 3) % 3]; n += 1
                c.upload(evplp.BUF_VPL_ACCUM, acc)
            c.noise_fold(1)
            states.append(c.download(evplp.BUF_VPL_ACCUM))
        assert np.isinf(states[-1][ONE[0], ONE[1], 0]) and not np.isfinite(states[-1][8 * ALL[0]:8 * ALL[0] + 8, 8 * ALL[1]:8 * ALL[1] + 8, :3]).all(-1).any()
        s = 1.0 / RETIRE_AT
        case = tracked_case(evplp, c, states, (1,) * RETIRE_AT)
        comp, noise = c.resolve(s, s, 1.0)[:RH], c.adaptive_tile_noise(s)
        est = c.noise_estimate(s)
        rs = sh.restate(case, s, 1.0, False, comp, case.light[:RH])
        ref = sh.statement64(case, s, 1.0, False, comp, case.light[:RH])
        per_tile = sh.broken_per_tile(ref.broken)
        assert per_tile[0, 0] == 1 and per_tile[ALL] == 64 and per_tile.sum() == 65
        assert np.isnan(est[0]) and np.isnan(est[1]) and same_figures(est, rs.figs)      # the report says that it is broken
        assert np.isfinite(noise).all() and noise[ALL] == 0.0                             # the decision works around it
        assert sh.worst_ratio(noise, rs.tiles, 1e-12 * np.abs(rs.tiles) + 1e-300) <= 1.0, (noise, rs.tiles)
        rt = sh.worst_ratio(noise, ref.tiles, ref.tile_bars)
        note(f"retire {mode} tiles", "room", rt)
        assert rt <= 1.0
        sound = per_tile < sh.in_image_per_tile(RW, RH)
        tau, gap, bar = sh.pick_tau(ref.tiles[sound], ref.tile_bars[sound])
        print(f"{mode}: tau {tau:.4g} in a gap of {gap:.4g} = {gap / bar:.3g} bars; tile (0, 0) reads {noise[0, 0]:.6g}, statement64 over its 63 sound pixels {ref.tiles[0, 0]:.6g}")
        assert gap >= 100.0 * bar
        want = (ref.tiles <= tau) & sound
        assert 0 < want.sum() < sound.sum() and not want[ALL]
        assert c.adaptive_retire(s, tau, 2) == int(want.sum())
        room_iteration(evplp, c, room, mode, RETIRE_AT); c.noise_fold(1)
        tiles = c.adaptive_tiles()
        assert np.array_equal(tiles, np.where(want, RETIRE_AT, RETIRE_AT + 1))           # exactly statement64's tiles; the all-broken tile stays active
        # the frozen figure of the retired tiles, the tracker's of the active ones, at today's composite
        states.append(c.download(evplp.BUF_VPL_ACCUM))
        N = RETIRE_AT + 1
        s = 1.0 / N
        comp, noise = c.resolve(s, s, 1.0)[:RH], c.adaptive_tile_noise(s)
        active = sh.statement64(tracked_case(evplp, c, states, (1,) * N), s, 1.0, False, comp, case.light[:RH])
        f = (f64(f32(s)) * N) / RETIRE_AT
        frozen = sh.statement64(case, s, 1.0, False, comp, case.light[:RH], s2K=f * f * RETIRE_AT)
        ref_tiles, ref_bars = np.where(want, frozen.tiles, active.tiles), np.where(want, frozen.tile_bars, active.tile_bars)
        rt = sh.worst_ratio(noise, ref_tiles, ref_bars)
        note(f"retire {mode} frozen tiles", "room", rt)
        assert rt <= 1.0 and np.isfinite(noise).all() and noise[ALL] == 0.0
        plan = evplp.plan_budgets(noise, tiles, 16, 1, 0.0, 1.0)                         # the handoff: EVPLP_OK with NaN pixels in the frame
        assert plan.size == noise.size and (plan >= 1).all()
        assert np.isnan(c.noise_estimate(s)[0])


# ---- the path tracer's budget mode: every tile is priced by its own n_t, K_t, B_t.  The raw sums R start as the accumulator at
# evplp_adaptive_enable_pt(ctx, 2), so the poison is uploaded before it; a plain context that replays the subsequence a tile of budget b
# takes (tests/test_gpu_pt_budget.py holds R to exactly that) gives the tile's sums at its folds
WARM, SAMPLES = 2, 2
BUDGET_ONES, BUDGET_ALL = ((3, 2), (3, 18)), (1, 2)          # single +Inf pixels in tiles (0, 0) and (0, 2); the all-broken tile


def test_pt_budget_mode_prices_every_tile_by_its_own_batches(evplp):
    from test_gpu_adaptive import tile_mask
    from test_gpu_pt_batch import jitters_of, seeds_of
    room = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=RW / RH)
    cam = room.cam_origin
    TX, TY = sh.tiles_of(RW, RH)
    budgets = (np.arange(TX * TY, dtype=np.int32) % 3).reshape(TY, TX)       # 0 (k_t = 0 at the later folds), 1, 2 of SAMPLES = 2
    assert budgets[0, 0] == 0 and budgets[0, 2] == 2 and budgets[BUDGET_ALL] == 1
    warm = [(jitters_of(1, RW, RH, 70 + i), seeds_of(1, i)) for i in range(WARM)]
    calls = [(jitters_of(SAMPLES, RW, RH, 5 + i), seeds_of(SAMPLES, WARM + SAMPLES * i)) for i in range(2)]
    N = WARM + 2 * SAMPLES
    s = 1.0 / N

    def poison(rows):
        acc = np.zeros((rows, RW, 4), f32)
        for y, x in BUDGET_ONES:
            acc[y, x, 0] = np.inf
        n = 0
        for y in range(8 * BUDGET_ALL[0], 8 * BUDGET_ALL[0] + 8):
            for x in range(8 * BUDGET_ALL[1], 8 * BUDGET_ALL[1] + 8):
                acc[y, x, n % 3] = (np.inf, -np.inf, np.nan)[(n // 3) % 3]; n += 1
        return acc

    with evplp.Context(RW, RH, 1, 1, 1) as c:
        room.upload(c)
        c.clear_accumulators(); c.upload(evplp.BUF_VPL_ACCUM, poison(c.local_rows)); c.noise_track(True); c.adaptive_enable(True, budget=True)
        for J, R in warm:
            c.path_trace_batch(cam, J, R, 3); c.noise_fold(1)
        c.adaptive_set_budgets(budgets)
        for J, R in calls:
            c.path_trace_batch(cam, J, R, 3); c.noise_fold(SAMPLES)
        tiles = c.adaptive_tiles()
        assert np.array_equal(tiles, WARM + 2 * budgets)
        comp, noise, var, est = c.resolve(s, s, 1.0)[:RH], c.adaptive_tile_noise(s), c.noise_variance(s)[:RH], c.noise_estimate(s)
        light, photon = c.download(evplp.BUF_LIGHT), c.download(evplp.BUF_PHOTON_ACCUM)
    assert np.isnan(est[0]) and np.isnan(est[1])
    assert np.isfinite(noise).all() and (noise >= 0).all() and noise[BUDGET_ALL] == 0.0 and noise[0, 0] > 0 and noise[0, 2] > 0
    plan = evplp.plan_budgets(noise, tiles, 16, 1, 0.0, 1.0)                 # EVPLP_OK with NaN pixels in the frame
    assert plan.size == noise.size and (plan >= 1).all()
    for b in (0, 1, 2):
        with evplp.Context(RW, RH, 1, 1, 1) as r:
            room.upload(r)
            r.clear_accumulators(); r.upload(evplp.BUF_VPL_ACCUM, poison(r.local_rows))
            states = [r.download(evplp.BUF_VPL_ACCUM)]
            for J, R in warm:
                r.path_trace_batch(cam, J, R, 3); states.append(r.download(evplp.BUF_VPL_ACCUM))
            for J, R in (calls if b else []):
                r.path_trace_batch(cam, J[:b], R[:b], 3); states.append(r.download(evplp.BUF_VPL_ACCUM))
        ks = (1,) * WARM + ((b, b) if b else ())
        n_t = WARM + 2 * b
        case = SimpleNamespace(family="room", W=RW, H=RH, variant=0, rows=light.shape[0], states=states, photon=photon, light=light, mask=None,
                               schedule=ks, K=n_t, B=len(ks))
        f = (f64(f32(s)) * N) / n_t
        ref = sh.statement64(case, s, 1.0, False, comp, light[:RH], s2K=f * f * n_t)      # the tile's own n_t, K_t = n_t, B_t
        sel = budgets == b
        rt = sh.worst_ratio(noise[sel], ref.tiles[sel], ref.tile_bars[sel])
        mine = SimpleNamespace(**{**vars(ref), "broken": ref.broken | ~tile_mask(sel, RW, RH)})
        rv = sh.variance_ratio(var, mine)
        note("pt budget tiles", f"budget {b}", rt); note("pt budget variance", f"budget {b}", rv)
        assert rt <= 1.0 and rv <= 1.0, (b, rt, rv)
        assert (sh.broken_per_tile(ref.broken)[sel] > 0).sum() == 1


def test_gather_budget_mode_prices_every_tile_by_its_own_batches(evplp):
    """evplp_adaptive_enable(ctx, 2): a window of 2 calls, budgets 0 / 1 / 2 by tile, a fold after every call -- a tile that sits a call out
    has k_t = 0 at that fold.  The poison and the per-budget reference runs as in the path tracer's test above."""
    from test_gpu_adaptive import tile_mask
    room = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=RW / RH)
    TX, TY = sh.tiles_of(RW, RH)
    budgets = (np.arange(TX * TY, dtype=np.int32) % 3).reshape(TY, TX)
    WINDOW, WINDOWS = 2, 2
    N = WARM + WINDOW * WINDOWS
    s = 1.0 / N
    taken = lambda b: list(range(WARM)) + [WARM + WINDOW * k + p for k in range(WINDOWS) for p in range(b)]

    def poison(rows):
        acc = np.zeros((rows, RW, 4), f32)
        for y, x in BUDGET_ONES:
            acc[y, x, 0] = np.inf
        n = 0
        for y in range(8 * BUDGET_ALL[0], 8 * BUDGET_ALL[0] + 8):
            for x in range(8 * BUDGET_ALL[1], 8 * BUDGET_ALL[1] + 8):
                acc[y, x, n % 3] = (np.inf, -np.inf, np.nan)[(n // 3) % 3]; n += 1
        return acc

    with evplp.Context(RW, RH, 32, 32, 4, deterministic=True) as c:
        room.upload(c)
        c.clear_accumulators(); c.upload(evplp.BUF_VPL_ACCUM, poison(c.local_rows)); c.noise_track(True)
        c.adaptive_enable(True, gather_budget=True); c.adaptive_budget_window(WINDOW)
        for i in range(N):
            if i == WARM:
                c.adaptive_set_budgets(budgets)
            room_iteration(evplp, c, room, "gather", i); c.noise_fold(1)
        tiles = c.adaptive_tiles()
        assert np.array_equal(tiles, WARM + WINDOWS * budgets)
        comp, noise, var, est = c.resolve(s, s, 1.0)[:RH], c.adaptive_tile_noise(s), c.noise_variance(s)[:RH], c.noise_estimate(s)
        light, photon = c.download(evplp.BUF_LIGHT), c.download(evplp.BUF_PHOTON_ACCUM)
    assert np.isnan(est[0]) and np.isnan(est[1])
    assert np.isfinite(noise).all() and (noise >= 0).all() and noise[BUDGET_ALL] == 0.0 and noise[0, 0] > 0 and noise[0, 2] > 0
    plan = evplp.plan_budgets(noise, tiles, WINDOW, 1, 0.0, 1.0)             # EVPLP_OK with NaN pixels in the frame
    assert plan.size == noise.size and (plan >= 1).all()
    for b in (0, 1, 2):
        with evplp.Context(RW, RH, 32, 32, 4, deterministic=True) as r:
            room.upload(r)
            r.clear_accumulators(); r.upload(evplp.BUF_VPL_ACCUM, poison(r.local_rows))
            states = [r.download(evplp.BUF_VPL_ACCUM)]
            for i in taken(b):
                room_iteration(evplp, r, room, "gather", i); states.append(r.download(evplp.BUF_VPL_ACCUM))
        n_t = WARM + WINDOWS * b
        case = SimpleNamespace(family="room", W=RW, H=RH, variant=0, rows=light.shape[0], states=states, photon=photon, light=light, mask=None,
                               schedule=(1,) * n_t, K=n_t, B=n_t)
        f = (f64(f32(s)) * N) / n_t
        ref = sh.statement64(case, s, 1.0, False, comp, light[:RH], s2K=f * f * n_t)
        sel = budgets == b
        rt = sh.worst_ratio(noise[sel], ref.tiles[sel], ref.tile_bars[sel])
        mine = SimpleNamespace(**{**vars(ref), "broken": ref.broken | ~tile_mask(sel, RW, RH)})
        rv = sh.variance_ratio(var, mine)
        note("gather budget tiles", f"budget {b}", rt); note("gather budget variance", f"budget {b}", rv)
        assert rt <= 1.0 and rv <= 1.0, (b, rt, rv)
