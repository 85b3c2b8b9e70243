"""Gather budget mode (evplp_adaptive_enable(ctx, 2), evplp_adaptive_budget_window, their evplp_group_* forms and photonfam's
"adaptive.budget" block) against what include/evplp.h writes down.  Everything is compared as bytes or doubles.

The 96 x 64 room of tests/test_gpu_convergence.py (NL 2048, NV 40, P 4) and a 100 x 52 frame of it for ragged edge tiles.  WARM iterations
with a fold each, then budgets 0 / 2 / 4 by tile index % 3 under a window of S = 4, two windows, a fold after every call.  A tile of budget b
takes the calls at phases 0 .. b - 1 of each window, so its raw sum R must equal, bit for bit, what a context with adaptivity off accumulates
from the warm-up plus exactly that subsequence of (jitter, light-path seed); the accumulator is (float)((double)R * (N / n_t)), each operation
rounded; the noise figures are noise_var_retired restated in numpy fp64."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import scenes
from test_gpu_convergence import NL, NV, P

pytestmark = pytest.mark.gpu

W, H = 96, 64
ODD = (100, 52)
WARM, S, WINDOWS = 4, 4, 2
CLASSES = (0, 2, 4)
N = WARM + S * WINDOWS                           # 12 accumulating gather calls
GBUF = ("BUF_GBUF_POSITION", "BUF_GBUF_NORMAL", "BUF_GBUF_DIFFUSE", "BUF_GBUF_PHONG")
f64, f32 = np.float64, np.float32


def class_map(w, h):
    ty, tx = (h + 7) // 8, (w + 7) // 8
    return np.array(CLASSES, np.int32)[np.arange(ty * tx) % 3].reshape(ty, tx)


def tile_mask(tiles, w, h):
    return np.kron(tiles, np.ones((8, 8), bool))[:h, :w].astype(bool)


def jitter_of(i):
    return (0.002 + 0.0004 * i, -0.001 + 0.0003 * i)


def taken(b):
    """the iterations a tile of budget b takes: the warm-up, then phases 0 .. b - 1 of every window"""
    return list(range(WARM)) + [WARM + S * k + p for k in range(WINDOWS) for p in range(min(b, S))]


class Room:
    def __init__(self, evplp, d, w, h):
        self.w, self.h = w, h
        self.jp = evplp.synth_scene(str(d), "room", 3000, 3, w, h, style="hard")
        self.sd, _ = scenes.load_obj_scene(self.jp)
        with evplp.Context(w, h, NL, NV, P) as m:
            m.load_scene_json(self.jp); self.bsr, self.total, _ = m.scene_metrics()

    def params(self, evplp, i, vsl=False):
        r = 0.05 * self.bsr
        fp = evplp.frame_params(camera_pos=self.sd.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), clamping_value=1.0 / self.total,
                                photon_radius=r, num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=i,
                                jitter=jitter_of(i))
        if vsl:
            fp.vsl_radius = r; fp.vsl_inv_pi_radius2 = 1.0 / (math.pi * r * r)
        return fp

    def context(self, evplp, **kw):
        c = evplp.Context(self.w, self.h, NL, NV, P, deterministic=True, **kw)
        c.load_scene_json(self.jp)
        return c

    def iteration(self, evplp, c, i, vsl=False):
        """one iteration; returns the call's (shadow rays, unoccluded pairs) where the runner has pass counters"""
        group = isinstance(c, evplp.Group)
        c.primary(jitter_of(i)); c.trace_light_paths(i)
        fp = self.params(evplp, i, vsl)
        if group:
            c.gather(fp, 1 if vsl else 0); return None
        (c.gather_vsl if vsl else c.gather_vpl)(fp)
        st = c.pass_stats(evplp.PASS_GATHER_VSL if vsl else evplp.PASS_GATHER_VPL)
        return st["rays"], st["shaded"]


def reference_run(evplp, room, b, vsl=False):
    """adaptivity off: the subsequence a tile of budget b sees, from a cleared accumulator.  The accumulator after each of its iterations, the
    per-iteration counters, and (b = S: the plain run of all N iterations) the last G-buffer and the light plane"""
    with room.context(evplp) as c:
        c.clear_accumulators()
        at, stats = [], {}
        for i in taken(b):
            stats[i] = room.iteration(evplp, c, i, vsl)
            at.append(c.download(evplp.BUF_VPL_ACCUM)[:room.h].copy())
        planes = {k: c.download(getattr(evplp, k))[:room.h].copy() for k in GBUF + ("BUF_LIGHT",)}
    return dict(at=at, stats=stats, planes=planes)


def start(c, window=S):
    c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, gather_budget=True)
    if window is not None:
        c.adaptive_budget_window(window)


def mixed_run(evplp, room, c, budgets, vsl=False, after_warm=None):
    """the mode: the warm-up, the budgets, WINDOWS windows of S calls, a fold after every call; returns the per-call counters"""
    start(c)
    stats = []
    for i in range(WARM):
        stats.append(room.iteration(evplp, c, i, vsl)); c.noise_fold(1)
    if after_warm:
        after_warm(c)
    c.adaptive_set_budgets(budgets)
    for i in range(WARM, N):
        stats.append(room.iteration(evplp, c, i, vsl)); c.noise_fold(1)
    return stats


def check_mixed(evplp, room, c, refs, what=""):
    w, h = room.w, room.h
    cls = class_map(w, h)
    acc = c.download(evplp.BUF_VPL_ACCUM)[:h]
    assert np.array_equal(c.adaptive_tiles(), WARM + WINDOWS * cls)
    assert np.array_equal(c.adaptive_budgets(), cls)
    for b in CLASSES:
        pm = tile_mask(cls == b, w, h)
        n_t = WARM + WINDOWS * b
        R = refs[b]["at"][-1]
        want = (R.astype(f64) * (f64(N) / f64(n_t))).astype(f32)
        diff = int((acc[pm] != want[pm]).sum())
        print(f"{what}{w}x{h} budget {b}: {int(pm.sum())} pixels, {diff} values differ from (float)(R * {N} / {n_t}); R max {R.max():.4g}")
        assert pm.any() and R.any()
        assert acc[pm].tobytes() == want[pm].tobytes(), (b, diff)


_shared = {}


def shared(evplp, tmp_path_factory, w, h):
    """the room at one size and the per-class reference runs (b = S is the plain run), computed once for the module"""
    if (w, h) not in _shared:
        room = Room(evplp, tmp_path_factory.mktemp(f"gather_budget_{w}"), w, h)
        _shared[(w, h)] = (room, {b: reference_run(evplp, room, b) for b in CLASSES})
    return _shared[(w, h)]


@pytest.fixture(scope="module", params=[(W, H), ODD], ids=["96x64", "100x52"])
def mixed(evplp, request, tmp_path_factory):
    return shared(evplp, tmp_path_factory, *request.param)


@pytest.fixture(scope="module")
def main(evplp, tmp_path_factory):
    return shared(evplp, tmp_path_factory, W, H)


@pytest.fixture(scope="module")
def ragged(evplp, tmp_path_factory):
    return shared(evplp, tmp_path_factory, *ODD)


def test_full_budgets_equal_the_plain_run(evplp, mixed):
    room, refs = mixed
    plain = refs[S]
    with room.context(evplp) as c:
        start(c, window=None)                                             # (the window's initial value: it must not matter)
        for i in range(N):
            st = room.iteration(evplp, c, i); c.noise_fold(1)
            assert st == plain["stats"][i] and st[0] > 0 and st[1] > 0, (i, st, plain["stats"][i])
            if i in (0, 5, N - 1):
                assert c.download(evplp.BUF_VPL_ACCUM)[:room.h].tobytes() == plain["at"][i].tobytes(), i
            assert np.array_equal(c.adaptive_tiles(), np.full_like(class_map(room.w, room.h), i + 1))
        assert (c.adaptive_budgets() == -1).all()
        assert plain["at"][-1].any()
        for k in GBUF + ("BUF_LIGHT",):
            assert c.download(getattr(evplp, k))[:room.h].tobytes() == plain["planes"][k].tobytes(), k
        assert not c.download(evplp.BUF_PHOTON_ACCUM).any()               # (no splat: the photon plane stays empty)


def test_mixed_budgets(evplp, mixed):
    room, refs = mixed
    cls = class_map(room.w, room.h)
    counts = [int((cls == b).sum()) for b in CLASSES]
    assert counts == ([32, 32, 32] if (room.w, room.h) == (W, H) else [31, 30, 30]), counts
    # 2 x 2 cut groups mix takers and skippers: some group holds more than one class
    g = [set(cls[y:y + 2, x:x + 2].ravel().tolist()) for y in range(0, cls.shape[0], 2) for x in range(0, cls.shape[1], 2)]
    assert any(len(s) > 1 for s in g)
    with room.context(evplp) as c:
        mixed_run(evplp, room, c, cls)
        check_mixed(evplp, room, c, refs)
        # G-buffer and light plane: every call runs its whole-frame primary, as in the plain run
        for k in GBUF + ("BUF_LIGHT",):
            assert c.download(getattr(evplp, k))[:room.h].tobytes() == refs[S]["planes"][k].tobytes(), k
        # a clear resets the records: every budget full again, n_t = 0
        c.clear_accumulators()
        assert (c.adaptive_budgets() == -1).all() and not c.adaptive_tiles().any()


@pytest.mark.parametrize("k", [1, 2, 4])
def test_splits_per_wave_change_no_bit(evplp, main, k):
    room, refs = main
    with room.context(evplp, gather_splits_per_wave=k) as c:
        mixed_run(evplp, room, c, class_map(room.w, room.h))
        check_mixed(evplp, room, c, refs, f"k = {k}: ")


def test_a_calibrating_gather_still_follows_the_schedule(evplp, mixed):
    """evplp_calibrate_blocks: the self-clocking kernels walk every tile; the reduce takes the scheduled tiles only"""
    room, refs = mixed
    with room.context(evplp) as c:
        mixed_run(evplp, room, c, class_map(room.w, room.h), after_warm=lambda c: c.calibrate_blocks(True))
        check_mixed(evplp, room, c, refs, "calibrating: ")


@pytest.mark.parametrize("size, b", [("main", 0), ("main", 1), ("main", 3), ("main", 9), ("ragged", 2)])
def test_uniform_budget_counters(evplp, request, size, b):
    room, refs = request.getfixturevalue(size)
    plain = refs[S]["stats"]
    with room.context(evplp) as c:
        stats = mixed_run(evplp, room, c, np.full_like(class_map(room.w, room.h), b))
        for i in range(WARM, N):
            phase = (i - WARM) % S
            want = plain[i] if phase < min(b, S) else (0, 0)
            print(f"{room.w}x{room.h} b = {b}, call {i} (phase {phase}): rays, pairs {stats[i]} / plain {plain[i]}")
            assert stats[i] == want, (i, stats[i], want)
        assert np.array_equal(c.adaptive_tiles(), np.full_like(class_map(room.w, room.h), WARM + WINDOWS * min(b, S)))


def test_window_and_set_budgets_restart_the_phase(evplp, main):
    """m counts from the last set_budgets / budget_window: a tile of budget 1 under S = 4 takes the call right after either"""
    room, refs = main
    ones = np.ones_like(class_map(room.w, room.h))
    with room.context(evplp) as c:
        start(c)
        for i in range(WARM):
            room.iteration(evplp, c, i); c.noise_fold(1)
        c.adaptive_set_budgets(ones)
        took = []
        for i, act in zip(range(WARM, WARM + 6), (None, None, "set", None, "window", None)):
            if act == "set":
                c.adaptive_set_budgets(ones)
            if act == "window":
                c.adaptive_budget_window(3)
            before = int(c.adaptive_tiles()[0, 0])
            st = room.iteration(evplp, c, i); c.noise_fold(1)
            took.append(int(c.adaptive_tiles()[0, 0]) - before)
            assert (st[0] > 0) == bool(took[-1])
        assert took == [1, 0, 1, 0, 1, 0], took


def variance_restated(at_fold, scale):
    """noise_var_retired of a tile whose folds closed one call each, fp64 in the kernels' order: (h, w, 3) doubles.  at_fold: the raw sums R at
    the tile's folds (after the cast to fp32); n_t = K_t = B_t = len(at_fold)"""
    prev = np.zeros_like(at_fold[0][..., :3])
    Q = np.zeros(prev.shape, f64)
    for R in at_fold:
        D = (R[..., :3] - prev)
        assert D.dtype == f32
        D = D.astype(f64)
        Q = Q + (D * D) / f64(1.0)
        prev = R[..., :3]
    Ssum = (prev - np.zeros_like(prev)).astype(f64)
    n_t = f64(len(at_fold)); K_t = n_t; B1 = f64(len(at_fold)) - f64(1.0)
    f = (f64(f32(scale)) * f64(N)) / n_t
    s2K = (f * f) * K_t
    v = (Q - (Ssum * Ssum) / K_t) / B1
    return s2K * np.where(v > 0.0, v, 0.0)


def test_noise_is_the_written_formula(evplp, mixed):
    room, refs = mixed
    w, h = room.w, room.h
    cls = class_map(w, h)
    scale = 1.0 / N
    with room.context(evplp) as c:
        mixed_run(evplp, room, c, cls)
        var = c.noise_variance(scale)[:h]
        want = np.zeros((h, w, 3), f64)
        for b in CLASSES:
            pm = tile_mask(cls == b, w, h)
            want[pm] = variance_restated(refs[b]["at"], scale)[pm]
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
        # the tiles at noise level tau are exactly the tiles the planner stops
        tau = float(np.sort(got.ravel())[got.size // 2])
        plan = evplp.plan_budgets(got, c.adaptive_tiles(), S, 1, tau, 1.0).reshape(cls.shape)
        assert 0 < (got <= tau).sum() < got.size
        assert np.array_equal(plan == 0, got <= tau)
        assert plan[got > tau].min() >= 1 and plan.max() <= S


def test_vsl(evplp, ragged):
    room, _ = ragged
    refs = {b: reference_run(evplp, room, b, vsl=True) for b in CLASSES}
    with room.context(evplp) as c:
        stats = mixed_run(evplp, room, c, class_map(room.w, room.h), vsl=True)
        check_mixed(evplp, room, c, refs, "VSL ")
        assert stats[0] == refs[S]["stats"][0] and stats[0][0] > 0


def strips_run(evplp, room, c, group, dealt=False):
    if group:
        c.load_scene_json(room.jp)
    if dealt:
        c.calibrate(True); room.iteration(evplp, c, 0); c.rebalance()
    mixed_run(evplp, room, c, class_map(room.w, room.h))
    s1 = 1.0 / N
    return {"accum": c.resolve(1.0, 0.0, 0.0)[:room.h] if group else c.download(evplp.BUF_VPL_ACCUM)[:room.h][..., :3],
            "tiles": c.adaptive_tiles(), "budgets": c.adaptive_budgets(), "tile_noise": c.adaptive_tile_noise(s1), "est": c.noise_estimate(s1),
            "var": c.noise_variance(s1)[:room.h]}


@pytest.fixture(scope="module")
def one_context(evplp, main):
    room, _ = main
    with room.context(evplp) as c:
        return strips_run(evplp, room, c, False)


@pytest.mark.parametrize("ranks, dealt", [(2, False), (2, True), (4, False), (4, True)])
def test_strips_equal_one_context(evplp, main, one_context, ranks, dealt):
    room, _ = main
    ref = one_context
    assert np.array_equal(ref["tiles"], WARM + WINDOWS * class_map(W, H)) and ref["tile_noise"].max() > 0
    with evplp.Group(W, H, NL, NV, P, ranks, devices=[0] * ranks, deterministic=True) as g:
        got = strips_run(evplp, room, g, True, dealt)
    assert np.ascontiguousarray(got["accum"]).tobytes() == np.ascontiguousarray(ref["accum"]).tobytes()
    assert np.array_equal(got["tiles"], ref["tiles"]) and np.array_equal(got["budgets"], ref["budgets"])
    assert got["tile_noise"].tobytes() == ref["tile_noise"].tobytes()
    assert got["est"] == ref["est"]
    assert got["var"].tobytes() == ref["var"].tobytes()


def _refused(evplp, calls):
    for k, call in enumerate(calls):
        with pytest.raises(evplp.EvplpError) as e:
            call()
        assert e.value.status == evplp.ERR_INVALID, k


def test_refusals_leave_the_context_usable(evplp, main):
    room, refs = main
    cls = class_map(W, H)
    cam = room.sd.cam_origin
    J, R = np.zeros((1, 2), np.float32), np.array([1], np.uint32)
    with room.context(evplp) as c, room.context(evplp) as off:
        # outside the mode: adaptivity off, and mode 1
        off.clear_accumulators()
        _refused(evplp, [lambda: off.adaptive_budget_window(4)])
        off.noise_track(True); off.adaptive_enable(True)
        _refused(evplp, [lambda: off.adaptive_budget_window(4), lambda: off.adaptive_set_budgets(cls)])
        # entering: no noise tracking; a photon splat since the last clear
        c.clear_accumulators()
        _refused(evplp, [lambda: c.adaptive_enable(True, gather_budget=True)])
        c.primary(jitter_of(0)); c.trace_light_paths(0); c.splat_photons(room.params(evplp, 0))
        c.noise_track(True)
        _refused(evplp, [lambda: c.adaptive_enable(True, gather_budget=True)])
        start(c)                                                          # (the clear forgets the splat)
        assert c._lib.evplp_adaptive_budget_window(None, 4) == evplp.ERR_INVALID

        def refusals(n_positive):
            before = c.download(evplp.BUF_VPL_ACCUM).copy()
            tiles, budgets = c.adaptive_tiles(), c.adaptive_budgets()
            fp0 = room.params(evplp, 1); fp0.do_accumulate = 0
            calls = [lambda: c.splat_photons(room.params(evplp, 1)), lambda: c.gather_lvc(room.params(evplp, 1)), lambda: c.path_trace(cam, 1, 3),
                     lambda: c.path_trace_batch(cam, J, R, 3), lambda: c.gather_vpl(fp0), lambda: c.gather_vsl(fp0),
                     lambda: c.adaptive_retire(1.0, 0.1, 2), lambda: c.adaptive_budget_window(0), lambda: c.adaptive_budget_window(65)]
            if n_positive:
                calls += [lambda: c.adaptive_enable(False), lambda: c.adaptive_enable(True), lambda: c.adaptive_enable(True, gather_budget=True),
                          lambda: c.adaptive_enable(True, budget=True), lambda: c.noise_track(False), lambda: c.noise_track(True)]
            _refused(evplp, calls)
            assert c.download(evplp.BUF_VPL_ACCUM).tobytes() == before.tobytes()
            assert np.array_equal(tiles, c.adaptive_tiles()) and np.array_equal(budgets, c.adaptive_budgets())

        refusals(False)
        _refused(evplp, [lambda: c.adaptive_set_budgets(cls)])           # no fold yet
        for i in range(WARM - 1):
            room.iteration(evplp, c, i); c.noise_fold(1)
        room.iteration(evplp, c, WARM - 1)
        refusals(True)
        _refused(evplp, [lambda: c.adaptive_set_budgets(cls)])           # a call unfolded: K != N
        c.noise_fold(1)
        c.adaptive_budget_window(S)                                       # (a refused window left the old one)
        # ... and the context goes on to exactly what an undisturbed run gives
        c.adaptive_set_budgets(cls)
        for i in range(WARM, N):
            room.iteration(evplp, c, i); c.noise_fold(1)
            if i == WARM + 1:
                refusals(True)
        check_mixed(evplp, room, c, refs, "after the refusals: ")
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True) as g:
        g.load_scene_json(room.jp)
        g.clear_accumulators()
        _refused(evplp, [lambda: g.adaptive_enable(True, gather_budget=True), lambda: g.adaptive_budget_window(4)])
        g.primary(jitter_of(0)); g.trace_light_paths(0); g.splat_photons(room.params(evplp, 0))
        g.noise_track(True)
        _refused(evplp, [lambda: g.adaptive_enable(True, gather_budget=True)])           # a splat since the last clear
        start(g)
        assert g._lib.evplp_group_adaptive_budget_window(None, 4) == evplp.ERR_INVALID
        for i in range(WARM):
            room.iteration(evplp, g, i); g.noise_fold(1)
        fp0 = room.params(evplp, 1); fp0.do_accumulate = 0
        _refused(evplp, [lambda: g.splat_photons(room.params(evplp, 1)), lambda: g.gather(room.params(evplp, 1), 2), lambda: g.gather(fp0, 0),
                         lambda: g.path_trace(cam, 1, 3), lambda: g.path_trace_batch(cam, J, R, 3), lambda: g.adaptive_retire(1.0, 0.1, 2),
                         lambda: g.adaptive_budget_window(0), lambda: g.adaptive_budget_window(65), lambda: g.adaptive_enable(False),
                         lambda: g.adaptive_enable(True), lambda: g.adaptive_enable(True, gather_budget=True), lambda: g.adaptive_enable(True, budget=True),
                         lambda: g.noise_track(False), lambda: g.noise_track(True)])
        g.adaptive_set_budgets(cls)                                       # the failures were not sticky
        room.iteration(evplp, g, WARM); g.noise_fold(1)
        assert np.array_equal(g.adaptive_tiles(), WARM + (cls > 0)) and np.array_equal(g.adaptive_budgets(), cls)
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True, partition="iterations") as g:
        g.load_scene_json(room.jp)
        g.clear_accumulators(); g.noise_track(True)
        _refused(evplp, [lambda: g.adaptive_enable(True, gather_budget=True), lambda: g.adaptive_budget_window(4)])
        room.iteration(evplp, g, 0)                                       # the group stays usable
        assert np.isfinite(g.resolve(1.0, 0.0, 1.0)).all()


# ---- the technique loop: photonfam's "adaptive": {"budget": {..}}
ITERS_T, WINDOW_T, EVERY_T, BATCH_T = 24, 4, 4, 2


def _block(jp_src, d, evplp, **over):
    d.mkdir()
    src = os.path.dirname(jp_src)
    for f in os.listdir(src):                                             # the scene's files next to the new JSON
        if not f.endswith(".json"):
            (d / f).write_bytes(open(os.path.join(src, f), "rb").read())
    root = json.load(open(jp_src))
    root["photonfam"].update(numMaxIteration=ITERS_T, numLightPaths=NL, numVplLightPaths=NV, radiusPercentage=0.05, misMode="balance", useJitter=False,
                             DoProgressive=False, deterministic=True, combinedFilename="c.pfm", weightedPhotonFilename="pm.pfm",
                             weightedVplFilename="vpl.pfm", statFilename="s.json", run=dict(photonSplat=False),
                             noise={"batchIterations": BATCH_T, "everyIterations": EVERY_T, "filename": "noise.json"},
                             adaptive={"tileRelMse": 0.0, "everyIterations": EVERY_T, "minBatches": 2, "iterationsFilename": "iters.pfm",
                                       "budget": {"window": WINDOW_T, "minSamples": 1, "referenceQuantile": 0.9}})
    for k, v in over.items():
        if isinstance(v, dict) and isinstance(root["photonfam"].get(k), dict):
            root["photonfam"][k].update(v)
        else:
            root["photonfam"][k] = v
    jp = d / "room.json"
    json.dump(root, open(jp, "w"))
    return str(jp), root


def test_technique_loop_equals_the_binding(evplp, main, tmp_path):
    room, _ = main
    d = tmp_path / "budget"
    jp, root = _block(room.jp, d, evplp)
    evplp.render_json(jp)
    got = np.ascontiguousarray(evplp.load_pfm(str(d / "c.pfm")))
    iters = evplp.load_pfm(str(d / "iters.pfm"))
    cps = json.load(open(d / "noise.json"))["checkpoints"]
    ntiles = class_map(W, H).size
    # the same sequence through the binding, with the loop's own fp32 parameters
    off = int(root["photonfam"]["rngOffset"])
    r = f32(room.bsr) * f32(0.05)
    pdf_mc = f32(NV) / f32(NL) * f32(0.318309886183790671537767526745028724068919291480912897495) / (r * r)
    samples = []
    with room.context(evplp) as c:
        start(c, window=WINDOW_T)
        for i in range(ITERS_T):
            fp = evplp.frame_params(camera_pos=room.sd.cam_origin, mis_mode="balance", pdf_mc=float(pdf_mc), clamping_value=float(f32(1.0) / f32(room.total)),
                                    photon_radius=float(r), num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1,
                                    rng_seed=i + off, jitter=(0.0, 0.0))
            c.primary((0.0, 0.0)); c.trace_light_paths(i + off); c.gather_vpl(fp)
            n = i + 1
            if n % BATCH_T == 0:
                c.noise_fold(BATCH_T)
                if n % EVERY_T == 0 and n // BATCH_T >= 2:
                    scale = float(f32(1.0) / f32(n))
                    plan = evplp.plan_budgets(c.adaptive_tile_noise(scale), c.adaptive_tiles(), WINDOW_T, 1, 0.0, 0.9)
                    c.adaptive_set_budgets(plan.reshape(class_map(W, H).shape))
                    samples.append((n, int(plan.sum())))
        s = float(f32(1.0) / f32(ITERS_T))
        want = np.ascontiguousarray(c.resolve(s, s, 1.0)[:H][::-1])
        tiles = c.adaptive_tiles()
    print(f"budgetSamples per plan: {samples}; n_t {tiles.min()} .. {tiles.max()} of {ITERS_T}")
    assert tiles.min() < ITERS_T and tiles.max() == ITERS_T                # some tile runs below the full rate, the reference tile at it
    assert got.tobytes() == want.tobytes()
    want_iters = np.kron(tiles[::-1], np.ones((8, 8)))[:H, :W]
    assert np.array_equal(iters[..., 0], (want_iters.astype(f64) / f64(ITERS_T)).astype(f32))
    by_iter = {p["iteration"]: p for p in cps}
    assert all("budgetSamples" in p and p["retiredTiles"] + p["activeTiles"] == ntiles for p in cps)
    for n, total in samples:
        assert by_iter[n]["budgetSamples"] == total, (n, by_iter[n], total)
    assert by_iter[EVERY_T]["budgetSamples"] == (samples[0][1] if samples[0][0] == EVERY_T else ntiles * WINDOW_T)


def test_technique_refusals(evplp, main, tmp_path):
    room, _ = main
    cases = {"photons": dict(run=dict(photonSplat=True)),
             "every": dict(adaptive={"everyIterations": 6}, noise={"batchIterations": 2, "everyIterations": 6}),
             "window": dict(adaptive={"budget": {"window": 65}}),
             "min": dict(adaptive={"budget": {"window": 4, "minSamples": 5}})}
    for name, over in cases.items():
        d = tmp_path / name
        jp, _ = _block(room.jp, d, evplp, **over)
        with pytest.raises(evplp.EvplpError) as e:
            evplp.render_json(jp)
        print(name, "->", e.value)
        assert "adaptive" in str(e.value), (name, str(e.value))
    # lvcphotonfam takes no "adaptive" block at all
    d = tmp_path / "lvc"
    jp, root = _block(room.jp, d, evplp)
    root["lvcphotonfam"] = root.pop("photonfam")
    json.dump(root, open(jp, "w"))
    with pytest.raises(evplp.EvplpError) as e:
        evplp.render_json(jp)
    assert "lvcphotonfam" in str(e.value), str(e.value)
