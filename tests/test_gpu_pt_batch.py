"""Batched path tracing (evplp_path_trace_batch, evplp_group_path_trace_batch and the pt technique's "samplesPerCall") against the sequence
it stands for:  for s: primary(jitters[s], 0); path_trace(camera, seeds[s], bounces, accumulate).

Everything is compared exactly.  The box room of tests/scenes.py at 96 x 64 and at 100 x 52 (neither side a multiple of 8): accumulator,
G-buffer planes, light plane and the pass counters for S = 1, 3, 8, from cleared and from filled accumulators; the same under scratch bounds
that force three chunks, chunks that end inside a tile's samples (S + 3 slots for S = 8; in path-trace adaptive mode too, with some tiles
retired) and one (tile, sample) per chunk; path-trace adaptive mode with some and with all tiles retired (active tiles bit for
bit, retired ones at the fp64 rescale, the noise figures as doubles); row strips of 2 and 4 virtual ranks, round robin and dealt, against one
context; every refusal; and the technique loop with samplesPerCall 4 against samplesPerCall 1, plain and adaptive, byte for byte."""
import json

import numpy as np
import pytest

import scenes
from test_gpu_adaptive import one_iteration
from test_gpu_convergence import NL, NV, P, params, room as synth_room, write_inputs

pytestmark = pytest.mark.gpu

W, H = 96, 64
ODD = (100, 52)
BOUNCES = 3
GBUF = ("BUF_GBUF_POSITION", "BUF_GBUF_NORMAL", "BUF_GBUF_DIFFUSE", "BUF_GBUF_PHONG")
SLOT = 4096                                   # bytes of one (tile, sample) of staging


def jitters_of(n, w, h, seed):
    """the reference's jitter: (2 u - 1) / resolution per axis"""
    u = np.random.default_rng(seed).random((n, 2))
    return ((2.0 * u - 1.0) / np.array([w, h], np.float64)).astype(np.float32)


def seeds_of(n, first):
    return np.arange(first, first + n, dtype=np.uint32)


def context(evplp, room, w=W, h=H):
    c = evplp.Context(w, h, 32, 32, 4, device=0, deterministic=True)
    room.upload(c)
    return c


def sequence(evplp, c, cam, J, R):
    """the S single calls; returns the summed path-trace counters"""
    rays = pairs = 0
    for j, r in zip(J, R):
        c.primary((float(j[0]), float(j[1]))); c.path_trace(cam, int(r), BOUNCES)
        st = c.pass_stats(evplp.PASS_PATH_TRACE)
        rays += st["rays"]; pairs += st["pairs"]
    return rays, pairs


def batch(evplp, c, cam, J, R):
    c.path_trace_batch(cam, J, R, BOUNCES)
    st = c.pass_stats(evplp.PASS_PATH_TRACE)
    return st["rays"], st["pairs"]


def planes(evplp, c, h):
    out = {"accum": c.download(evplp.BUF_VPL_ACCUM)[:h], "light": c.download(evplp.BUF_LIGHT)[:h]}
    for b in GBUF:
        out[b] = c.download(getattr(evplp, b))[:h]
    return out


def assert_same(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k] != b[k]).sum()))


@pytest.fixture(scope="module")
def room():
    return scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=W / H)


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_plain_batch_equals_the_sequence(evplp, w, h):
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    with context(evplp, box, w, h) as a, context(evplp, box, w, h) as b:
        for S in (1, 3, 8):
            a.clear_accumulators(); b.clear_accumulators()
            for part, first in (("cleared", 10 * S), ("filled", 10 * S + 100)):      # the second round starts from what the first left
                J, R = jitters_of(S, w, h, first), seeds_of(S, first)
                ca = sequence(evplp, a, cam, J, R)
                cb = batch(evplp, b, cam, J, R)
                pa, pb = planes(evplp, a, h), planes(evplp, b, h)
                print(f"{w}x{h} S={S} {part}: rays {ca[0]} / {cb[0]}, paths {ca[1]} / {cb[1]}, accumulator max {pa['accum'].max():.4g}")
                assert pa["accum"].any() and ca[1] > 0
                assert_same(pa, pb, (w, h, S, part))
                assert ca == cb, (S, part, ca, cb)


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_chunking_changes_no_bit(evplp, w, h):
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    S = 8
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    J0, R0, J1, R1 = jitters_of(S, w, h, 1), seeds_of(S, 1), jitters_of(S, w, h, 2), seeds_of(S, 50)
    with context(evplp, box, w, h) as a:
        ca = sequence(evplp, a, cam, J0, R0); ca2 = sequence(evplp, a, cam, J1, R1)
        want = planes(evplp, a, h)
    # a third of the slots (rounded down to whole entries): at least three chunks of entries; S + 3 slots: the chunks end inside a tile's
    # samples; then one slot: one (tile, sample) per chunk
    third = (tiles // 3) * S * SLOT
    assert -(-tiles // (third // SLOT // S)) >= 3
    for bound in (third, (S + 3) * SLOT, SLOT):
        with context(evplp, box, w, h) as b:
            b.path_trace_batch_scratch(bound)
            cb = batch(evplp, b, cam, J0, R0); cb2 = batch(evplp, b, cam, J1, R1)
            assert_same(want, planes(evplp, b, h), (w, h, bound))
            assert (ca, ca2) == (cb, cb2), (bound, ca, cb, ca2, cb2)
            # one byte less than one slot is refused, and the context goes on under a bound that fits
            b.path_trace_batch_scratch(SLOT - 1)
            with pytest.raises(evplp.EvplpError) as e:
                b.path_trace_batch(cam, J0, R0, BOUNCES)
            assert e.value.status == evplp.ERR_INVALID, e.value
            assert_same(want, planes(evplp, b, h), "a refused call changes nothing")
            b.path_trace_batch_scratch(bound)


def approx_tile_means(evplp, c, scale, w, h):
    """per-tile mean of the relative variance, as evplp_adaptive_retire forms it up to rounding (used only to PLACE tau in a wide gap)"""
    var = c.noise_variance(scale)[:h].astype(np.float64)
    cp = c.resolve(scale, scale, 1.0)[:h].astype(np.float64)
    rel = var.sum(axis=2) / ((cp * cp).sum(axis=2) + 0.001)
    ty, tx = (h + 7) // 8, (w + 7) // 8
    return np.array([[rel[y * 8:y * 8 + 8, x * 8:x * 8 + 8].mean() for x in range(tx)] for y in range(ty)])


def tau_in_a_gap(means):
    """between two neighbouring tile means near the median that lie at least 1 % apart: the device's own rounding cannot cross it"""
    m = np.sort(means.ravel())
    k = len(m) // 2
    for j in list(range(k, len(m) - 1)) + list(range(k - 1, 0, -1)):
        if m[j + 1] > m[j] * 1.01 + 1e-300:
            return 0.5 * (m[j] + m[j + 1])
    raise AssertionError("no gap between the tile means")


WARM = 4                                      # iterations (one fold each) before the retirement


def warm_up(c, cam, w, h, batched):
    """clear, track, path-trace mode, WARM iterations with a fold after each: single calls, or batches of one"""
    c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, path_trace=True)
    J, R = jitters_of(WARM, w, h, 77), seeds_of(WARM, 0)
    for i in range(WARM):
        if batched:
            c.path_trace_batch(cam, J[i:i + 1], R[i:i + 1], BOUNCES)
        else:
            c.primary((float(J[i][0]), float(J[i][1]))); c.path_trace(cam, int(R[i]), BOUNCES)
        c.noise_fold(1)


def tile_mask(retired, w, h):
    return np.kron(retired, np.ones((8, 8), bool))[:h, :w]


def adaptive_batch_against_the_sequence(evplp, w, h, S, bound=None):
    """path-trace adaptive mode, some tiles retired after the warm-up: one batched call of S (under the scratch bound, if given) against
    the S single calls"""
    box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)
    cam = box.cam_origin
    tx, ty = (w + 7) // 8, (h + 7) // 8
    J, R = jitters_of(S, w, h, 5), seeds_of(S, WARM)
    with context(evplp, box, w, h) as a, context(evplp, box, w, h) as b:
        warm_up(a, cam, w, h, False); warm_up(b, cam, w, h, True)
        assert_same(planes(evplp, a, h), planes(evplp, b, h), "warm-up")
        s0 = 1.0 / WARM
        tau = tau_in_a_gap(approx_tile_means(evplp, a, s0, w, h))
        na, nb = a.adaptive_retire(s0, tau, 2), b.adaptive_retire(s0, tau, 2)
        print(f"{w}x{h}: tau {tau:.6g} retires {na} of {tx * ty} tiles")
        assert 0 < na < tx * ty and na == nb                              # a fraction strictly between 0 and 1, not assumed
        snap = b.download(evplp.BUF_VPL_ACCUM)[:h].copy()                 # R: the accumulator at retirement
        ca = sequence(evplp, a, cam, J, R); a.noise_fold(S)
        if bound is not None:
            b.path_trace_batch_scratch(bound)
        cb = batch(evplp, b, cam, J, R); b.noise_fold(S)
        ta, tb = a.adaptive_tiles(), b.adaptive_tiles()
        assert np.array_equal(ta, tb)
        retired = ta == WARM                                              # n_t of a retired tile; an active one reports N = WARM + S
        assert int(retired.sum()) == na and np.array_equal(ta, np.where(retired, WARM, WARM + S))
        pm = tile_mask(retired, w, h)
        pa, pb = planes(evplp, a, h), planes(evplp, b, h)
        assert pa["accum"][~pm].tobytes() == pb["accum"][~pm].tobytes()   # active tiles: bit for bit
        assert pa["light"][~pm].tobytes() == pb["light"][~pm].tobytes()
        want = (snap.astype(np.float64) * (np.float64(WARM + S) / np.float64(WARM))).astype(np.float32)
        assert pb["accum"][pm].tobytes() == want[pm].tobytes()            # retired tiles: the fp64 rescale
        assert pb["accum"].tobytes() == pa["accum"].tobytes()             # ... which is what the sequence leaves
        lit = pm & (pb["light"] != 0).any(axis=2)
        assert pb["light"][lit].tobytes() == pa["light"][lit].tobytes()   # retired tiles' light plane: every non-zero pixel is the sequence's
        for k in GBUF:
            assert pa[k].tobytes() == pb[k].tobytes(), k
        assert ca == cb and 0 < ca[1], (ca, cb)
        s1 = 1.0 / (WARM + S)
        assert a.noise_estimate(s1) == b.noise_estimate(s1)               # doubles, frozen figures of the retired tiles included
        assert a.noise_variance(s1)[:h].tobytes() == b.noise_variance(s1)[:h].tobytes()


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_adaptive_batch_equals_the_sequence(evplp, w, h):
    adaptive_batch_against_the_sequence(evplp, w, h, 3)


@pytest.mark.parametrize("w, h", [(W, H), ODD])
def test_adaptive_chunking_changes_no_bit(evplp, w, h):
    """S = 8 under S + 3 slots: the chunks end inside an active tile's samples, and the retired tiles have no items at all"""
    adaptive_batch_against_the_sequence(evplp, w, h, 8, (8 + 3) * SLOT)


def test_every_tile_retired(evplp, room):
    cam = room.cam_origin
    S = 3
    J, R = jitters_of(S, W, H, 9), seeds_of(S, WARM)
    with context(evplp, room) as a, context(evplp, room) as b:
        warm_up(a, cam, W, H, False); warm_up(b, cam, W, H, True)
        tiles = ((W + 7) // 8) * ((H + 7) // 8)
        assert a.adaptive_retire(1.0 / WARM, 1e300, 2) == tiles and b.adaptive_retire(1.0 / WARM, 1e300, 2) == tiles
        snap = b.download(evplp.BUF_VPL_ACCUM)[:H].copy()
        assert sequence(evplp, a, cam, J, R) == (0, 0)
        assert batch(evplp, b, cam, J, R) == (0, 0)                       # nothing traced
        pa, pb = planes(evplp, a, H), planes(evplp, b, H)
        want = (snap.astype(np.float64) * (np.float64(WARM + S) / np.float64(WARM))).astype(np.float32)
        assert pb["accum"].tobytes() == want.tobytes() == pa["accum"].tobytes()
        for k in GBUF:                                                    # the call still leaves the last jitter's G-buffer
            assert pa[k].tobytes() == pb[k].tobytes(), k
        lit = (pb["light"] != 0).any(axis=2)
        assert pb["light"][lit].tobytes() == pa["light"][lit].tobytes()
        assert np.array_equal(a.adaptive_tiles(), b.adaptive_tiles())


@pytest.fixture(scope="module")
def scene(evplp, tmp_path_factory):
    d = tmp_path_factory.mktemp("pt_batch_scene")
    jp = synth_room(evplp, d)
    sd, _ = scenes.load_obj_scene(jp)
    return jp, sd


def adaptive_run(evplp, c, jp, sd, tau, group, dealt=False):
    """path-trace mode through the batch alone: WARM batches of one with a fold each, a retirement, one batch of three, a fold"""
    cam = sd.cam_origin
    c.load_scene_json(jp)
    if dealt:
        with evplp.Context(W, H, NL, NV, P) as m:
            m.load_scene_json(jp); bsr, total, _ = m.scene_metrics()
        c.calibrate(True); one_iteration(c, params(evplp, sd, bsr, total, 0), 0, True); c.rebalance()
    warm_up(c, cam, W, H, True)
    s0 = 1.0 / WARM
    out = {}
    if tau is None:
        tau = tau_in_a_gap(approx_tile_means(evplp, c, s0, W, H))
    out["tau"] = tau
    out["retired"] = c.adaptive_retire(s0, tau, 2)
    S = 3
    c.path_trace_batch(cam, jitters_of(S, W, H, 5), seeds_of(S, WARM), BOUNCES); c.noise_fold(S)
    s1 = 1.0 / (WARM + S)
    out["tiles"] = c.adaptive_tiles()
    out["accum"] = c.resolve(1.0, 0.0, 0.0)[:H] if group else c.download(evplp.BUF_VPL_ACCUM)[:H][..., :3]
    out["light"] = c.resolve(0.0, 0.0, 1.0)[:H] if group else c.download(evplp.BUF_LIGHT)[:H][..., :3]
    out["est"] = c.noise_estimate(s1)
    out["var"] = c.noise_variance(s1)[:H]
    return out


def test_plain_batch_equals_the_sequence_on_the_furnished_room(evplp, scene):
    """The synthetic room of the technique tests: more materials and longer paths than the box room.  It is the scene that showed a
    multiply-add of the sampled direction fused the other way round in pt_batch_trace_kernel (one unit in the last place in 17 - 43 of the
    6 144 pixels per sample); tests/test_pt_batch_same_arithmetic.py holds the cause at build time."""
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as a, evplp.Context(W, H, NL, NV, P, deterministic=True) as b:
        a.load_scene_json(jp); b.load_scene_json(jp)
        a.clear_accumulators(); b.clear_accumulators()
        for S, first in ((1, 3), (4, 20), (8, 40)):
            J, R = jitters_of(S, W, H, first), seeds_of(S, first)
            ca = sequence(evplp, a, sd.cam_origin, J, R)
            cb = batch(evplp, b, sd.cam_origin, J, R)
            assert_same(planes(evplp, a, H), planes(evplp, b, H), ("room", S))
            assert ca == cb and ca[1] > 0, (S, ca, cb)


@pytest.fixture(scope="module")
def one_context(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        return adaptive_run(evplp, c, jp, sd, None, False)


@pytest.mark.parametrize("ranks, dealt", [(2, False), (2, True), (4, False), (4, True)])
def test_strips_equal_one_context(evplp, scene, one_context, ranks, dealt):
    jp, sd = scene
    ref = one_context
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert 0 < ref["retired"] < tiles
    with evplp.Group(W, H, NL, NV, P, ranks, devices=[0] * ranks, deterministic=True) as g:
        got = adaptive_run(evplp, g, jp, sd, ref["tau"], True, dealt)
    assert got["retired"] == ref["retired"] and np.array_equal(got["tiles"], ref["tiles"])
    assert np.ascontiguousarray(got["accum"]).tobytes() == np.ascontiguousarray(ref["accum"]).tobytes()
    # the light plane: active tiles bit for bit; a retired tile's non-zero pixels as one context's
    pm = tile_mask(ref["tiles"] == WARM, W, H)
    assert got["light"][~pm].tobytes() == ref["light"][~pm].tobytes()
    assert got["light"].tobytes() == ref["light"].tobytes()               # (strips retire the same tiles: the whole plane agrees)
    assert got["est"] == ref["est"]
    assert got["var"].tobytes() == ref["var"].tobytes()


def _refused(evplp, calls):
    for call in calls:
        with pytest.raises(evplp.EvplpError) as e:
            call()
        assert e.value.status == evplp.ERR_INVALID, e.value


def test_refusals_leave_the_context_usable(evplp, room, scene):
    import ctypes as C
    cam = room.cam_origin
    J, R = jitters_of(3, W, H, 1), seeds_of(3, 1)
    bad = J.copy(); bad[1, 0] = np.nan
    cp = (C.c_float * 3)(*[float(v) for v in cam])
    with context(evplp, room) as a, context(evplp, room) as b:
        a.path_trace_batch(cam, J, R, BOUNCES)
        want = planes(evplp, a, H)
        L = b._lib
        _refused(evplp, [lambda: b.path_trace_batch(cam, np.zeros((0, 2), np.float32), np.zeros(0, np.uint32), BOUNCES),
                         lambda: b.path_trace_batch(cam, jitters_of(65, W, H, 1), seeds_of(65, 0), BOUNCES),
                         lambda: b.path_trace_batch(cam, bad, R, BOUNCES)])
        for args in ((None, 3, J.ctypes.data, R.ctypes.data), (C.byref(cp), 3, None, R.ctypes.data), (C.byref(cp), 3, J.ctypes.data, None),
                     (C.byref(cp), -1, J.ctypes.data, R.ctypes.data)):
            assert L.evplp_path_trace_batch(b._h, args[0], args[1], args[2], args[3], BOUNCES) == evplp.ERR_INVALID
        b.path_trace_batch_scratch(SLOT - 1)
        _refused(evplp, [lambda: b.path_trace_batch(cam, J, R, BOUNCES)])
        b.path_trace_batch_scratch(1 << 30)
        b.noise_track(True); b.adaptive_enable(True)                      # gather mode: refused as evplp_path_trace is
        _refused(evplp, [lambda: b.path_trace_batch(cam, J, R, BOUNCES), lambda: b.path_trace(cam, 1, BOUNCES)])
        b.adaptive_enable(False); b.noise_track(False)
        assert not b.download(evplp.BUF_VPL_ACCUM).any()                  # nothing was accumulated by a refused call
        b.path_trace_batch(cam, J, R, BOUNCES)                            # ... and a correct call gives what it gives a fresh context
        assert_same(want, planes(evplp, b, H), "after the refusals")
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c, evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True) as g:
        c.load_scene_json(jp); g.load_scene_json(jp)
        c.clear_accumulators(); g.clear_accumulators()
        c.path_trace_batch(sd.cam_origin, J, R, BOUNCES)
        gp = (C.c_float * 3)(*[float(v) for v in sd.cam_origin])
        _refused(evplp, [lambda: g.path_trace_batch(sd.cam_origin, np.zeros((0, 2), np.float32), np.zeros(0, np.uint32), BOUNCES),
                         lambda: g.path_trace_batch(sd.cam_origin, jitters_of(65, W, H, 1), seeds_of(65, 0), BOUNCES),
                         lambda: g.path_trace_batch(sd.cam_origin, bad, R, BOUNCES)])
        assert g._lib.evplp_group_path_trace_batch(g._h, C.byref(gp), 3, None, R.ctypes.data, BOUNCES) == evplp.ERR_INVALID
        assert g._lib.evplp_group_path_trace_batch(g._h, C.byref(gp), 3, J.ctypes.data, None, BOUNCES) == evplp.ERR_INVALID
        g.path_trace_batch_scratch(SLOT - 1)
        _refused(evplp, [lambda: g.path_trace_batch(sd.cam_origin, J, R, BOUNCES)])
        g.path_trace_batch_scratch(64 * SLOT)                             # (and a small bound on every rank: chunks)
        g.noise_track(True); g.adaptive_enable(True)
        _refused(evplp, [lambda: g.path_trace_batch(sd.cam_origin, J, R, BOUNCES)])
        g.adaptive_enable(False); g.noise_track(False)
        g.path_trace_batch(sd.cam_origin, J, R, BOUNCES)                  # the failures were not sticky: the group renders, as one context
        assert g.resolve(1.0, 0.0, 0.0)[:H].tobytes() == np.ascontiguousarray(c.download(evplp.BUF_VPL_ACCUM)[:H][..., :3]).tobytes()


def _render(evplp, d, jp_src, **block):
    write_inputs(evplp, d, jp_src)
    root = json.load(open(jp_src))
    root.pop("photonfam")
    root["pt"] = dict(rngOffset=3, numMaxIteration=10, timeLimitMs=1e9, frameMode="accumulate", outputFilename="c.pfm", statFilename="s.json",
                      useJitter=True, useStat=True, numSamplePerPixel=1, numMaxBounces=3)
    root["pt"].update(block)
    jp = d / "room.json"
    json.dump(root, open(jp, "w"))
    evplp.render_json(str(jp))
    return open(d / "c.pfm", "rb").read(), json.load(open(d / "s.json"))


def test_technique_block(evplp, scene, tmp_path):
    jp, _ = scene
    # adaptivity off, a trimmed last batch (4 + 4 + 2): the PFM of samplesPerCall 1, byte for byte
    one, st1 = _render(evplp, tmp_path / "one", jp)
    four, st4 = _render(evplp, tmp_path / "four", jp, samplesPerCall=4)
    assert st1["numIterations"] == st4["numIterations"] == 10
    assert one == four
    # adaptive: tau = the image's mean relMSE at the retirement (iteration 8, two folds of four), so some tiles retire and some do not
    noise = {"batchIterations": 4, "everyIterations": 4, "filename": "noise.json"}
    _render(evplp, tmp_path / "probe", jp, noise=noise)
    cps = json.load(open(tmp_path / "probe" / "noise.json"))["checkpoints"]
    tau = [p for p in cps if p["iteration"] == 8][0]["relMse"]
    block = {"tileRelMse": tau, "everyIterations": 4, "minBatches": 2, "iterationsFilename": "iters.pfm"}
    outs = {}
    for S in (1, 4):
        d = tmp_path / f"adaptive{S}"
        img, st = _render(evplp, d, jp, noise=noise, adaptiveSampling=block, samplesPerCall=S)
        outs[S] = (img, open(d / "iters.pfm", "rb").read(), json.load(open(d / "noise.json"))["checkpoints"], st["numIterations"])
    retired = outs[1][2][-1]["retiredTiles"]
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    print(f"tau {tau:.6g}: {retired} of {tiles} tiles retired at iteration 8")
    assert 0 < retired < tiles
    assert outs[1][3] == outs[4][3] == 10
    assert outs[1][0] == outs[4][0]                                       # the image
    assert outs[1][1] == outs[4][1]                                       # the per-tile iteration map
    assert [(p["iteration"], p["retiredTiles"], p["relMse"]) for p in outs[1][2]] == [(p["iteration"], p["retiredTiles"], p["relMse"]) for p in outs[4][2]]
    assert outs[1][0] != one                                              # (and retirement did change the image)
