"""Budget mode of the path tracer (evplp_adaptive_enable_pt(ctx, 2), evplp_adaptive_set_budgets / _budgets / _tile_noise, their evplp_group_*
forms, evplp_plan_budgets in the pt technique's "adaptiveSampling.budget") against what include/evplp.h writes down.

Everything is compared as bytes or doubles.  The box room of tests/scenes.py at 96 x 64 and at 100 x 52, 3 bounces.  A tile that takes the
first s_t samples of every call must hold, as its raw sum R, exactly what a context with adaptivity off accumulates from that subsequence of
(jitter, seed); the accumulator is R at the fp64 rescale N / n_t; the noise figures are the written formula, restated in numpy fp64."""
import ctypes as C
import json

import numpy as np
import pytest

import scenes
from test_gpu_adaptive import one_iteration
from test_gpu_convergence import NL, NV, P, params, room as synth_room
from test_gpu_pt_batch import BOUNCES, GBUF, ODD, SLOT, H, W, _refused, _render, assert_same, batch, context, jitters_of, planes, seeds_of, sequence, tile_mask

pytestmark = pytest.mark.gpu

WARM = 4                                      # full samples, one call and one fold each, before the budgets are set
S = 4                                         # samples of the two budgeted calls
CLASSES = (0, 2, 4)                           # the budget of image tile i is CLASSES[i % 3]
f64, f32 = np.float64, np.float32


def class_map(w, h):
    """(tile rows, tile columns) int32: the budget of every image tile"""
    ty, tx = (h + 7) // 8, (w + 7) // 8
    return np.array(CLASSES, np.int32)[np.arange(ty * tx) % 3].reshape(ty, tx)


def samples_of(w, h):
    """the (jitters, seeds) of the WARM single-sample calls and of the two calls of S"""
    warm = [(jitters_of(1, w, h, 77 + i), seeds_of(1, i)) for i in range(WARM)]
    calls = [(jitters_of(S, w, h, 5), seeds_of(S, WARM)), (jitters_of(S, w, h, 6), seeds_of(S, WARM + S))]
    return warm, calls


def start(c):
    c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, budget=True)


def mixed_run(evplp, c, cam, w, h, budgets, after_warm=None):
    """budget mode: the warm-up, the budgets, the two calls with a fold after each; returns the summed path-trace counters of the two calls"""
    warm, calls = samples_of(w, h)
    start(c)
    for J, R in warm:
        c.path_trace_batch(cam, J, R, BOUNCES); c.noise_fold(1)
    if after_warm:
        after_warm(c)
    c.adaptive_set_budgets(budgets)
    rays = pairs = 0
    for J, R in calls:
        if isinstance(c, evplp.Group):                                    # (a group has no pass counters of its own)
            c.path_trace_batch(cam, J, R, BOUNCES); c.noise_fold(S)
            continue
        r, p = batch(evplp, c, cam, J, R); c.noise_fold(S)
        rays += r; pairs += p
    return rays, pairs


def reference_run(evplp, c, cam, w, h, b):
    """adaptivity off: the subsequence a tile of budget b sees, from a cleared accumulator; the accumulator at every fold that closes
    samples for such a tile, and the counters of the two calls' parts"""
    warm, calls = samples_of(w, h)
    c.clear_accumulators()
    at_fold, rays, pairs = [], 0, 0
    for J, R in warm:
        c.path_trace_batch(cam, J, R, BOUNCES)
        at_fold.append(c.download(evplp.BUF_VPL_ACCUM)[:h].copy())
    for J, R in calls:
        if b > 0:
            r, p = batch(evplp, c, cam, J[:b], R[:b])
            rays += r; pairs += p
            at_fold.append(c.download(evplp.BUF_VPL_ACCUM)[:h].copy())
    return at_fold, (rays, pairs)


def variance_restated(at_fold, b, scale):
    """noise_var_retired of a tile of budget b, fp64 in the kernels' order: (H, W, 3) doubles.  at_fold: the raw sums at the tile's folds.
    The contract's record: WARM folds of k = 1, then (b > 0) two folds of k = b; n_t = K_t = WARM + 2 b, B_t = WARM + (2 if b else 0)."""
    ks = [1] * WARM + ([b, b] if b > 0 else [])
    assert len(ks) == len(at_fold)
    prev = np.zeros_like(at_fold[0][..., :3])
    Q = np.zeros(prev.shape, f64)
    for k, R in zip(ks, at_fold):
        D = (R[..., :3] - prev).astype(f64)                               # fp32 subtraction, then widened
        assert (R[..., :3] - prev).dtype == f32
        Q = Q + (D * D) / f64(k)
        prev = R[..., :3]
    Ssum = (prev - np.zeros_like(prev)).astype(f64)                       # c_prev - c_start (fp32), c_start = the cleared accumulator
    n_t = f64(WARM + 2 * b); K_t = n_t; B1 = f64(len(ks)) - f64(1.0)
    N = f64(WARM + 2 * S)
    f = (f64(f32(scale)) * N) / n_t
    s2K = (f * f) * K_t
    v = (Q - (Ssum * Ssum) / K_t) / B1
    return s2K * np.where(v > 0.0, v, 0.0)


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_full_budgets_equal_the_plain_batch(evplp, w, h):
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    with context(evplp, box, w, h) as a, context(evplp, box, w, h) as b:
        a.clear_accumulators(); start(b)
        n = 0
        for k, first in ((1, 10), (3, 30), (8, 80)):
            J, R = jitters_of(k, w, h, first), seeds_of(k, first)
            ca = batch(evplp, a, cam, J, R)
            cb = batch(evplp, b, cam, J, R); b.noise_fold(k)
            n += k
            pa, pb = planes(evplp, a, h), planes(evplp, b, h)
            print(f"{w}x{h} S={k}: rays {ca[0]} / {cb[0]}, paths {ca[1]} / {cb[1]}, accumulator max {pa['accum'].max():.4g}")
            assert pa["accum"].any() and ca[1] > 0
            assert_same(pa, pb, (w, h, k))
            assert ca == cb, (k, ca, cb)
            assert np.array_equal(b.adaptive_tiles(), np.full(((h + 7) // 8, (w + 7) // 8), n, np.int32))
            assert (b.adaptive_budgets() == -1).all()


def check_mixed(evplp, c, refs, full, w, h):
    """the budget context after mixed_run against the per-class references and the full sequence"""
    cls = class_map(w, h)
    N = WARM + 2 * S
    acc = c.download(evplp.BUF_VPL_ACCUM)[:h]
    tiles = c.adaptive_tiles()
    assert np.array_equal(tiles, WARM + 2 * cls)
    assert np.array_equal(c.adaptive_budgets(), cls)
    for b in CLASSES:
        pm = tile_mask(cls == b, w, h)
        assert pm.any()
        R = refs[b][0][-1]
        want = (R.astype(f64) * (f64(N) / f64(WARM + 2 * b))).astype(f32)
        diff = int((acc[pm] != want[pm]).sum())
        print(f"{w}x{h} budget {b}: {int(pm.sum())} pixels, {diff} differ from (float)(R * {N} / {WARM + 2 * b})")
        assert acc[pm].tobytes() == want[pm].tobytes(), (b, diff)
    pf = planes(evplp, full, h)
    light = c.download(evplp.BUF_LIGHT)[:h]
    lit = (light != 0).any(axis=2)
    assert light[lit].tobytes() == pf["light"][lit].tobytes()             # every non-zero light pixel is the full sequence's
    for k in GBUF:                                                        # the G-buffer of the last jitter's primary
        assert c.download(getattr(evplp, k))[:h].tobytes() == pf[k].tobytes(), k


@pytest.fixture(scope="module", params=[(W, H), ODD], ids=["96x64", "100x52"])
def mixed(evplp, request):
    """the per-class reference runs and the full sequence, shared by the tests of the mixed budgets"""
    w, h = request.param
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    refs = {}
    for b in CLASSES:
        with context(evplp, box, w, h) as r:
            refs[b] = reference_run(evplp, r, cam, w, h, b)
    full = context(evplp, box, w, h)
    reference_run(evplp, full, cam, w, h, S)
    yield w, h, box, cam, refs, full
    full.close()


def test_mixed_budgets(evplp, mixed):
    w, h, box, cam, refs, full = mixed
    cls = class_map(w, h)
    counts = [int((cls == b).sum()) for b in CLASSES]
    assert counts == ([32, 32, 32] if (w, h) == (W, H) else [31, 30, 30]), counts
    with context(evplp, box, w, h) as c:
        mixed_run(evplp, c, cam, w, h, cls)
        check_mixed(evplp, c, refs, full, w, h)


def test_uniform_budget_counters(evplp, mixed):
    w, h, box, cam, refs, full = mixed
    with context(evplp, box, w, h) as c:
        got = mixed_run(evplp, c, cam, w, h, np.full_like(class_map(w, h), 2))
        want = refs[2][1]
        print(f"{w}x{h} b = 2 of S = {S}: rays {got[0]} / {want[0]}, paths {got[1]} / {want[1]}")
        assert got == want and want[1] > 0
        N = WARM + 2 * S
        want_acc = (refs[2][0][-1].astype(f64) * (f64(N) / f64(WARM + 4))).astype(f32)
        assert c.download(evplp.BUF_VPL_ACCUM)[:h].tobytes() == want_acc.tobytes()


def test_chunking_changes_no_bit(evplp, mixed):
    w, h, box, cam, refs, full = mixed
    cls = class_map(w, h)
    needed = int(cls.sum())                                               # slots of a budgeted call: sum of s_t
    third = (needed // 3) * SLOT
    for bound in (third, 11 * SLOT, SLOT):                                # (11 slots: the chunks end inside the samples of the tiles of budget 4)
        with context(evplp, box, w, h) as c:
            c.path_trace_batch_scratch(bound)

            def one_byte_short(c):
                # one byte below one slot is refused and changes nothing; the context goes on under the bound that fits
                before = planes(evplp, c, h)
                c.path_trace_batch_scratch(SLOT - 1)
                J, R = jitters_of(S, w, h, 5), seeds_of(S, WARM)
                _refused(evplp, [lambda: c.path_trace_batch(cam, J, R, BOUNCES)])
                assert_same(before, planes(evplp, c, h), "a refused call changes nothing")
                assert np.array_equal(c.adaptive_tiles(), np.full_like(cls, WARM))
                c.path_trace_batch_scratch(bound)
            mixed_run(evplp, c, cam, w, h, cls, after_warm=one_byte_short)
            check_mixed(evplp, c, refs, full, w, h)


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_chunks_that_end_inside_a_tile_change_no_bit(evplp, w, h):
    """full budgets, S = 8 under S + 3 slots of staging, from the cleared and from the filled accumulator: the sequence of single calls of a
    context with adaptivity off, byte for byte, and its pass counters"""
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    S8 = 8
    with context(evplp, box, w, h) as a, context(evplp, box, w, h) as b:
        a.clear_accumulators(); start(b)
        b.path_trace_batch_scratch((S8 + 3) * SLOT)
        for first in (1, 50):
            J, R = jitters_of(S8, w, h, first), seeds_of(S8, first)
            ca = sequence(evplp, a, cam, J, R)
            cb = batch(evplp, b, cam, J, R); b.noise_fold(S8)
            print(f"{w}x{h} S={S8}, {S8 + 3} slots: rays {ca[0]} / {cb[0]}, paths {ca[1]} / {cb[1]}")
            assert_same(planes(evplp, a, h), planes(evplp, b, h), (w, h, first))
            assert ca == cb and ca[1] > 0, (first, ca, cb)


def test_noise_is_the_written_formula(evplp, mixed):
    """noise_variance against noise_var_retired restated in numpy fp64, bit for bit after the cast to float32; adaptive_tile_noise against the
    mean of rel recomputed from that variance and resolve, to 1e-12 relative (the tree's order is not restated).  The float32 image
    noise_variance returns cannot carry 1e-12, so rel is formed from the restatement's doubles -- the ones whose cast was just found equal."""
    w, h, box, cam, refs, full = mixed
    cls = class_map(w, h)
    scale = 1.0 / (WARM + 2 * S)
    with context(evplp, box, w, h) as c:
        mixed_run(evplp, c, cam, w, h, cls)
        var = c.noise_variance(scale)[:h]
        want = np.zeros((h, w, 3), f64)
        for b in CLASSES:
            pm = tile_mask(cls == b, w, h)
            # budget 0: B_t = WARM and Q holds the warm-up's folds alone -- the two later folds left the tile alone
            want[pm] = variance_restated(refs[b][0], b, scale)[pm]
            diff = int((var[pm] != want[pm].astype(f32)).sum())
            print(f"{w}x{h} budget {b}: variance max {want[pm].max():.4g}, {diff} values differ")
            assert var[pm].tobytes() == want[pm].astype(f32).tobytes(), (b, diff)
        assert want.max() > 0
        cp = c.resolve(scale, scale, 1.0)[:h].astype(f64)
        rel = ((want[..., 0] + want[..., 1]) + want[..., 2]) / (((cp[..., 0] * cp[..., 0] + cp[..., 1] * cp[..., 1]) + cp[..., 2] * cp[..., 2]) + 0.001)
        ty, tx = cls.shape
        means = np.array([[rel[y * 8:y * 8 + 8, x * 8:x * 8 + 8].mean() for x in range(tx)] for y in range(ty)])
        got = c.adaptive_tile_noise(scale)
        err = np.abs(got - means) / np.maximum(means, 1e-300)
        print(f"{w}x{h}: tile noise {means.min():.4g} .. {means.max():.4g}, largest relative difference {err.max():.3g}")
        assert means.max() > 0 and (err <= 1e-12).all(), float(err.max())


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_tile_noise_is_the_retirement_figure(evplp, w, h):
    """mode 1: a tile whose adaptive_tile_noise is <= tau is retired by adaptive_retire at that tau, and no other tile -- the same doubles,
    so tau is put ON a tile's figure"""
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    with context(evplp, box, w, h) as c:
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, path_trace=True)
        for J, R in samples_of(w, h)[0]:
            c.path_trace_batch(cam, J, R, BOUNCES); c.noise_fold(1)
        s0 = 1.0 / WARM
        t = c.adaptive_tile_noise(s0)
        tau = float(np.sort(t.ravel())[t.size // 2])
        want = t <= tau
        assert 0 < want.sum() < t.size
        assert c.adaptive_retire(s0, tau, 2) == int(want.sum())
        frozen = c.adaptive_tile_noise(s0)
        assert frozen.tobytes() == t.tobytes()                            # N unchanged: a retired tile's frozen figure is the one it retired at
        J, R = jitters_of(1, w, h, 5), seeds_of(1, WARM)
        c.path_trace_batch(cam, J, R, BOUNCES)
        assert np.array_equal(c.adaptive_tiles() == WARM, want)           # (an active tile now reports N = WARM + 1)


@pytest.fixture(scope="module")
def scene(evplp, tmp_path_factory):
    d = tmp_path_factory.mktemp("pt_budget_scene")
    jp = synth_room(evplp, d)
    sd, _ = scenes.load_obj_scene(jp)
    return jp, sd


def strips_run(evplp, c, jp, sd, group, dealt=False):
    c.load_scene_json(jp)
    if dealt:
        with evplp.Context(W, H, NL, NV, P) as m:
            m.load_scene_json(jp); bsr, total, _ = m.scene_metrics()
        c.calibrate(True); one_iteration(c, params(evplp, sd, bsr, total, 0), 0, True); c.rebalance()
    cls = class_map(W, H)
    mixed_run(evplp, c, sd.cam_origin, W, H, cls)
    s1 = 1.0 / (WARM + 2 * S)
    return {"accum": c.resolve(1.0, 0.0, 0.0)[:H] if group else c.download(evplp.BUF_VPL_ACCUM)[:H][..., :3],
            "tiles": c.adaptive_tiles(), "budgets": c.adaptive_budgets(), "tile_noise": c.adaptive_tile_noise(s1), "est": c.noise_estimate(s1)}


@pytest.fixture(scope="module")
def one_context(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        return strips_run(evplp, c, jp, sd, False)


@pytest.mark.parametrize("ranks, dealt", [(2, False), (2, True), (4, False), (4, True)])
def test_strips_equal_one_context(evplp, scene, one_context, ranks, dealt):
    jp, sd = scene
    ref = one_context
    assert np.array_equal(ref["tiles"], WARM + 2 * class_map(W, H)) and ref["tile_noise"].max() > 0
    with evplp.Group(W, H, NL, NV, P, ranks, devices=[0] * ranks, deterministic=True) as g:
        got = strips_run(evplp, g, jp, sd, True, dealt)
    assert np.ascontiguousarray(got["accum"]).tobytes() == np.ascontiguousarray(ref["accum"]).tobytes()
    assert np.array_equal(got["tiles"], ref["tiles"]) and np.array_equal(got["budgets"], ref["budgets"])
    assert got["tile_noise"].tobytes() == ref["tile_noise"].tobytes()
    assert got["est"] == ref["est"]


def test_refusals_leave_the_context_usable(evplp, mixed, scene):
    w, h, box, cam, refs, full = mixed
    cls = class_map(w, h)
    jp, sd = scene
    warm, calls = samples_of(w, h)
    with context(evplp, box, w, h) as c, context(evplp, box, w, h) as off:
        L = c._lib
        n = cls.size
        ok = np.ascontiguousarray(cls)
        out = np.zeros(n, np.float64)
        # outside budget mode: adaptivity off, and mode 1
        off.clear_accumulators()
        _refused(evplp, [lambda: off.adaptive_set_budgets(cls), lambda: off.adaptive_budgets(), lambda: off.adaptive_tile_noise(1.0)])
        off.noise_track(True); off.adaptive_enable(True, path_trace=True)
        _refused(evplp, [lambda: off.adaptive_set_budgets(cls), lambda: off.adaptive_budgets(), lambda: off.adaptive_tile_noise(1.0)])   # (no fold yet)
        # budget mode
        c.clear_accumulators()
        _refused(evplp, [lambda: c.adaptive_enable(True, budget=True)])   # no noise tracking
        start(c)
        fp = evplp.frame_params(camera_pos=cam, mis_mode=1, pdf_mc=1.0, photon_radius=0.4, num_light_paths=32, num_vpl_light_paths=32,
                                photons_per_path=4, rng_seed=3, jitter=(0.0, 0.0), do_accumulate=1)

        def refusals(set_ok, noise_ok):
            before = planes(evplp, c, h)
            tiles, budgets = c.adaptive_tiles(), c.adaptive_budgets()
            bad_hi, bad_lo = cls.copy(), cls.copy()
            bad_hi.flat[5] = 65; bad_lo.flat[7] = -1
            calls_ = [lambda: c.path_trace(cam, 1, BOUNCES), lambda: c.gather_vpl(fp), lambda: c.gather_vsl(fp), lambda: c.gather_lvc(fp),
                      lambda: c.adaptive_retire(1.0, 0.1, 2),
                      lambda: c.adaptive_set_budgets(bad_hi), lambda: c.adaptive_set_budgets(bad_lo),
                      lambda: c.adaptive_set_budgets(cls.ravel()[:-1]), lambda: c.adaptive_set_budgets(np.zeros(n + 1, np.int32))]
            if c.adaptive_tiles().max() > 0:                              # N > 0: no switch of the mode or of the tracker
                calls_ += [lambda: c.adaptive_enable(False), lambda: c.adaptive_enable(False, path_trace=True), lambda: c.adaptive_enable(True, path_trace=True),
                           lambda: c.adaptive_enable(True, budget=True), lambda: c.noise_track(False), lambda: c.noise_track(True)]
            if not set_ok:
                calls_ += [lambda: c.adaptive_set_budgets(cls)]
            if not noise_ok:
                calls_ += [lambda: c.adaptive_tile_noise(1.0)]
            _refused(evplp, calls_)
            assert L.evplp_adaptive_set_budgets(c._h, None, n) == evplp.ERR_INVALID
            assert L.evplp_adaptive_budgets(c._h, None, n) == evplp.ERR_INVALID
            assert L.evplp_adaptive_budgets(c._h, ok.ctypes.data, n - 1) == evplp.ERR_INVALID
            assert L.evplp_adaptive_tile_noise(c._h, C.c_float(1.0), C.c_float(1.0), 0, None, n) == evplp.ERR_INVALID
            assert L.evplp_adaptive_tile_noise(c._h, C.c_float(1.0), C.c_float(1.0), 0, out.ctypes.data, n - 1) == evplp.ERR_INVALID
            assert_same(before, planes(evplp, c, h), "a refused call changes no plane")
            assert np.array_equal(tiles, c.adaptive_tiles()) and np.array_equal(budgets, c.adaptive_budgets())

        refusals(False, False)                                            # N = 0, no fold
        c.path_trace_batch(cam, *warm[0], BOUNCES); c.noise_fold(1)
        refusals(False, False)                                            # one fold
        for J, R in warm[1:3]:
            c.path_trace_batch(cam, J, R, BOUNCES); c.noise_fold(1)
        c.path_trace_batch(cam, *warm[3], BOUNCES)
        refusals(False, True)                                             # three folds but a sample unfolded: K != N
        c.noise_fold(1)
        refusals(True, True)
        # ... and the context goes on to exactly what an undisturbed run gives
        c.adaptive_set_budgets(cls)
        for J, R in calls:
            c.path_trace_batch(cam, J, R, BOUNCES); c.noise_fold(S)
        check_mixed(evplp, c, refs, full, w, h)
        # a clear resets the records: every budget full again, n_t = 0
        c.clear_accumulators()
        assert (c.adaptive_budgets() == -1).all() and not c.adaptive_tiles().any()
    if (w, h) != (W, H):
        return
    gcls = class_map(W, H)
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True) as g:
        g.load_scene_json(jp)
        gcam = sd.cam_origin
        g.clear_accumulators()
        _refused(evplp, [lambda: g.adaptive_enable(True, budget=True)])   # no noise tracking
        g.noise_track(True); g.adaptive_enable(True, budget=True)
        _refused(evplp, [lambda: g.adaptive_set_budgets(gcls), lambda: g.adaptive_tile_noise(1.0)])       # no fold
        for J, R in warm:
            g.path_trace_batch(gcam, J, R, BOUNCES); g.noise_fold(1)
        bad = gcls.copy(); bad.flat[3] = 65
        _refused(evplp, [lambda: g.path_trace(gcam, 1, BOUNCES), lambda: g.gather(fp, 0), lambda: g.adaptive_retire(1.0, 0.1, 2),
                         lambda: g.adaptive_set_budgets(bad), lambda: g.adaptive_set_budgets(gcls.ravel()[:-1]),
                         lambda: g.adaptive_enable(False, path_trace=True), lambda: g.noise_track(False)])
        assert g._lib.evplp_group_adaptive_set_budgets(g._h, None, gcls.size) == evplp.ERR_INVALID
        assert g._lib.evplp_group_adaptive_budgets(g._h, None, gcls.size) == evplp.ERR_INVALID
        assert g._lib.evplp_group_adaptive_tile_noise(g._h, C.c_float(1.0), C.c_float(1.0), 0, None, gcls.size) == evplp.ERR_INVALID
        g.adaptive_set_budgets(gcls)                                      # the failures were not sticky
        g.path_trace_batch(gcam, *calls[0], BOUNCES); g.noise_fold(S)
        assert np.array_equal(g.adaptive_tiles(), WARM + gcls) and np.array_equal(g.adaptive_budgets(), gcls)
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True, partition="iterations") as g:
        g.load_scene_json(jp)
        g.clear_accumulators(); g.noise_track(True)
        _refused(evplp, [lambda: g.adaptive_enable(True, budget=True), lambda: g.adaptive_set_budgets(gcls), lambda: g.adaptive_budgets(),
                         lambda: g.adaptive_tile_noise(1.0)])
        g.path_trace_batch(sd.cam_origin, *calls[0], BOUNCES)             # the group stays usable
        assert np.isfinite(g.resolve(0.25, 0.0, 1.0)).all()


def _untimed(x):
    """a noise curve without its wall-clock fields (timeMs, overheadMs), which no two runs share"""
    if isinstance(x, dict):
        return {k: _untimed(v) for k, v in x.items() if not k.endswith("Ms")}
    if isinstance(x, list):
        return [_untimed(v) for v in x]
    return x


def test_technique_loop(evplp, scene, tmp_path):
    """pt with samplesPerCall 4, "budget": {} and tileRelMse 0 for 32 iterations on the furnished room"""
    jp, _ = scene
    noise = {"batchIterations": 4, "everyIterations": 4, "filename": "noise.json"}
    block = {"tileRelMse": 0, "everyIterations": 4, "budget": {}, "iterationsFilename": "iters.pfm"}
    plain, st = _render(evplp, tmp_path / "plain", jp, numMaxIteration=32, samplesPerCall=4)
    assert st["numIterations"] == 32
    outs = []
    for k in range(2):
        d = tmp_path / f"budget{k}"
        img, st = _render(evplp, d, jp, numMaxIteration=32, samplesPerCall=4, noise=noise, adaptiveSampling=block)
        assert st["numIterations"] == 32
        outs.append((img, open(d / "iters.pfm", "rb").read(), _untimed(json.load(open(d / "noise.json")))))
    assert outs[0][:2] == outs[1][:2]                                     # the same JSON twice: identical bytes
    assert outs[0][2] == outs[1][2]                                       # ... and the same curve, but for its wall-clock fields
    iters = evplp.load_image(str(tmp_path / "budget0" / "iters.pfm"))
    values = np.unique(iters)
    print(f"n_t / N: {len(values)} distinct values, {values.min():.4g} .. {values.max():.4g}")
    assert len(values) >= 2 and values.max() == 1.0
    a = evplp.load_image(str(tmp_path / "plain" / "c.pfm")).astype(f64)
    b = evplp.load_image(str(tmp_path / "budget0" / "c.pfm")).astype(f64)
    print(f"image mean: plain {a.mean():.6g}, budgets {b.mean():.6g}")
    assert abs(b.mean() - a.mean()) <= 0.02 * a.mean()
    cps = json.load(open(tmp_path / "budget0" / "noise.json"))["checkpoints"]
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert all("budgetSamples" in p and p["activeTiles"] == tiles and tiles <= p["budgetSamples"] <= 4 * tiles for p in cps), cps
    assert cps[-1]["budgetSamples"] < 4 * tiles                           # some tile runs below the full rate
