"""The statistics kernels and the gather's reduce on a ragged frame, 259 x 13.

Every other test of the plain noise and frame-error kernels runs at 96 x 64 (100 x 52 in budget mode): an even pixel count and W <= 256.
Here 259 > 256, so three threads of a row's workgroup take a second pixel (the row kernels' x += 256 loop); 259 % 8 = 3 and 13 rows give a
partial tile column and a partial tile row, and in strips of 8 rows the second rank holds 5 image rows of its 8.  What this frame does NOT
reach is the fold's lone last pixel (two == false in noise_fold_body): the fold runs over W * local_rows plane pixels, local_rows is a
multiple of 8 for every context (16 here, 8 per rank of the group), so the count is even whatever W and H are, and no call of the API can
make it odd.  The numpy restatements are those of tests/test_gpu_noise.py, test_gpu_convergence.py and
test_gpu_adaptive.py, with their tolerances: the variance image bit for bit, the figures to 1e-12."""
import math

import numpy as np
import pytest

import scenes
from test_gpu_adaptive import frozen_figures, rel_of, tile_mask
from test_gpu_convergence import close, numpy_error
from test_gpu_noise import numpy_figures, numpy_variance

pytestmark = pytest.mark.gpu

W, H = 259, 13
TX, TY = (W + 7) // 8, (H + 7) // 8                  # 33 x 2 = 66 tiles
NL, NV, P = 256, 16, 4
ITERS, SCHEDULE = 4, (1, 1, 2)
RETIRE_AT = 2
f32, f64 = np.float32, np.float64


def mask_top_down():
    mask = np.full((H, W, 3), 255, np.uint8)
    mask[3:6, :, :] = 0                              # a band of rows
    mask[8:12, 250:, :] = 0                          # a block of columns, the partial tile column among them
    mask[0, 256:, 0] = 0; mask[0, 256:, 2] = 0       # kept: one non-zero byte is enough (the pixels of the row kernels' second trip)
    return mask


def sums(evplp, c):
    return (c.download(evplp.BUF_VPL_ACCUM)[..., :3] + c.download(evplp.BUF_PHOTON_ACCUM)[..., :3]).astype(f32)[:H]


def test_uploaded_planes_against_numpy(evplp):
    """no scene: seeded random accumulators, uploaded before every "iteration"; rows past H hold large finite values that reach no figure"""
    rng = np.random.default_rng(259013)
    mask = mask_top_down()
    s = 1.0 / ITERS
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        rows = c.local_rows
        assert rows > H
        light = np.zeros((rows, W, 4), f32)
        lit = rng.random((rows, W)) < 0.1
        light[..., 0] = np.where(lit, rng.random((rows, W)), 0.0); light[..., 1] = light[..., 0] * f32(0.5); light[..., 2] = light[..., 0] * f32(0.25)
        light[H:] = f32(1.0e30)
        assert lit[:H].any() and not lit[:H].all()
        c.upload(evplp.BUF_LIGHT, light)
        acc = [np.zeros((rows, W, 4), f32), np.zeros((rows, W, 4), f32)]

        def next_iteration(j):
            for a in acc:
                a[:H, :, :3] += rng.random((H, W, 3)).astype(f32)
                a[H:] = f32(1.0e30) * f32(j + 1)
            c.upload(evplp.BUF_VPL_ACCUM, acc[0]); c.upload(evplp.BUF_PHOTON_ACCUM, acc[1])

        next_iteration(0)
        c.noise_track(True, mask)
        cs = [sums(evplp, c)]
        bounds, last = set(np.cumsum(SCHEDULE).tolist()), 0
        for it in range(1, ITERS + 1):
            next_iteration(it)
            cs.append(sums(evplp, c))
            if it in bounds:
                c.noise_fold(it - last); last = it
        var = numpy_variance(cs, SCHEDULE, s)
        assert var.max() > 0 and np.isfinite(var).all()
        assert c.noise_variance(s)[:H].tobytes() == var.astype(f32).tobytes()              # the variance image bit for bit
        got_light = c.download(evplp.BUF_LIGHT)[:H]
        est, est_me = c.noise_estimate(s), c.noise_estimate(s, 1.0, mask_emitter=True)
        print("noise_estimate", est, "mask_emitter", est_me)
        close(est, numpy_figures(var, c.resolve(s, s, 1.0)[:H], got_light, 1.0, False, mask), 1e-12)
        close(est_me, numpy_figures(var, c.resolve(s, s, 1.0, mask_emitter=True)[:H], got_light, 1.0, True, mask), 1e-12)
        assert est_me[0] < est[0] and est[2] != est[1]                                     # the emitter mask and the pixel mask both bite
        # the frame error of the same planes
        ref = rng.random((H, W, 3)).astype(f32)
        ref[0, 0] = 0.0; ref[12, 258] = 0.0; ref[5, 257] = 0.0           # |ref|^2 = 0: the 0.001 alone is the denominator
        for m in (None, mask):
            c.set_error_reference(ref, m)
            for mask_emitter in (False, True):
                img = c.resolve(s, s, 1.0, mask_emitter=mask_emitter)[:H]
                got = c.frame_error(s, s, 1.0, mask_emitter=mask_emitter)
                want = numpy_error(img, ref, m)
                print("frame_error", got)
                assert want[1] > 0 and np.isfinite(want).all()
                close(got, want, 1e-12)
        img = c.resolve(s, s, 1.0)[:H]
        c.set_error_reference(np.ascontiguousarray(img[::-1]), mask)
        assert c.frame_error(s, s, 1.0) == (0.0, 0.0, 0.0)                # the frame against itself


class Room:
    def __init__(self, evplp, d):
        self.jp = evplp.synth_scene(str(d), "room", 600, 1, W, H)
        self.sd, _ = scenes.load_obj_scene(self.jp)
        with evplp.Context(W, H, NL, NV, P) as m:
            m.load_scene_json(self.jp); self.bsr, self.total, _ = m.scene_metrics()

    def params(self, evplp, i):
        r = 0.05 * self.bsr
        return evplp.frame_params(camera_pos=self.sd.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), clamping_value=1.0 / self.total,
                                  photon_radius=r, num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=i,
                                  jitter=(0.002, -0.001))

    def iteration(self, evplp, c, i, splat=True):
        fp = self.params(evplp, i)
        c.primary((0.002, -0.001)); c.trace_light_paths(i)
        if isinstance(c, evplp.Group):
            c.gather(fp, 0)
        else:
            c.gather_vpl(fp)
        if splat:
            c.splat_photons(fp)


@pytest.fixture(scope="module")
def room(evplp, tmp_path_factory):
    return Room(evplp, tmp_path_factory.mktemp("stats_shapes"))


def tracked_run(evplp, room, c, ref):
    """ITERS iterations folded by SCHEDULE under the mask; the figures, and on a context the sums after every iteration"""
    own = isinstance(c, evplp.Context)
    s = 1.0 / ITERS
    c.clear_accumulators()
    c.noise_track(True, mask_top_down())
    cs = [sums(evplp, c)] if own else None
    bounds, last = set(np.cumsum(SCHEDULE).tolist()), 0
    for i in range(ITERS):
        room.iteration(evplp, c, i)
        if own:
            cs.append(sums(evplp, c))
        if i + 1 in bounds:
            c.noise_fold(i + 1 - last); last = i + 1
    c.set_error_reference(ref, mask_top_down())
    out = dict(cs=cs, est=c.noise_estimate(s), est_me=c.noise_estimate(s, 1.0, mask_emitter=True), var=c.noise_variance(s)[:H],
               err=c.frame_error(s, s, 1.0), err_me=c.frame_error(s, s, 1.0, mask_emitter=True, gamma=True))
    if own:
        out.update(composite=c.resolve(s, s, 1.0)[:H], light=c.download(evplp.BUF_LIGHT)[:H])
    return out


@pytest.fixture(scope="module")
def plain(evplp, room):
    """one context, adaptivity off: the run everything else here is compared with"""
    ref = np.random.default_rng(13).random((H, W, 3)).astype(f32)
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(room.jp)
        return dict(tracked_run(evplp, room, c, ref), ref=ref)


def test_the_room_against_numpy_and_two_strips(evplp, room, plain):
    mask = mask_top_down()
    var = numpy_variance(plain["cs"], SCHEDULE, 1.0 / ITERS)
    assert var.max() > 0
    assert plain["var"].tobytes() == var.astype(f32).tobytes()
    close(plain["est"], numpy_figures(var, plain["composite"], plain["light"], 1.0, False, mask), 1e-12)
    close(plain["err"], numpy_error(plain["composite"], plain["ref"], mask), 1e-12)
    print("one context:", plain["est"], plain["est_me"], plain["err"], plain["err_me"])
    assert plain["est"][1] > 0 and plain["err"][1] > 0
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0, 0], strip_rows=8, deterministic=True) as g:
        g.load_scene_json(room.jp)
        two = tracked_run(evplp, room, g, plain["ref"])
    for k in ("est", "est_me", "err", "err_me"):
        assert two[k] == plain[k], (k, two[k], plain[k])                                    # the same doubles
    assert two["var"].tobytes() == plain["var"].tobytes()


def test_retired_tiles_on_the_ragged_frame(evplp, room, plain):
    """Retirement after RETIRE_AT iterations at the median tile noise, then the rest of the run: the frozen variance and figures against the
    written formula (tests/test_gpu_adaptive.py test_frozen_noise_of_retired_pixels), an active tile's noise against numpy's mean of rel."""
    s = 1.0 / ITERS
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(room.jp)
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable()
        for i in range(RETIRE_AT):
            room.iteration(evplp, c, i); c.noise_fold(1)
        noise_at = c.adaptive_tile_noise(1.0 / RETIRE_AT)
        tau = float(np.median(noise_at))
        retired = noise_at <= tau
        print(f"tile noise after {RETIRE_AT} folds: min {noise_at.min():.4g}, median {tau:.4g}, max {noise_at.max():.4g}; {int(retired.sum())} of {retired.size} retire")
        assert retired.shape == (TY, TX) and 0 < retired.sum() < retired.size
        assert c.adaptive_retire(1.0 / RETIRE_AT, tau, 2) == int(retired.sum())
        for i in range(RETIRE_AT, ITERS):
            room.iteration(evplp, c, i)
        c.noise_fold(ITERS - RETIRE_AT)
        assert np.array_equal(c.adaptive_tiles(), np.where(retired, RETIRE_AT, ITERS))
        var, est, composite = c.noise_variance(s)[:H], c.noise_estimate(s), c.resolve(s, s, 1.0)[:H]
        tile_noise = c.adaptive_tile_noise(s)
    pm = tile_mask(retired, W, H)
    active_var = numpy_variance(plain["cs"], SCHEDULE, s)
    frozen, want = frozen_figures(plain["cs"], RETIRE_AT, ITERS, pm, active_var, composite, plain["light"])
    assert var[pm].tobytes() == frozen.astype(f32)[pm].tobytes()
    assert var[~pm].tobytes() == plain["var"][~pm].tobytes()              # active pixels as the plain run
    for g, w in zip(est, want):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1e-30), (est, want)
    # an active tile's figure: the mean of rel over its in-image pixels
    _, rel = rel_of(active_var, composite, plain["light"])
    for ty, tx in zip(*np.nonzero(~retired)):
        t = rel[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]
        assert abs(tile_noise[ty, tx] - t.sum() / t.size) <= 1e-12 * abs(t.sum() / t.size) + 1e-300, (ty, tx, t.shape)


def test_the_gather_reduce_on_the_ragged_frame(evplp, room, monkeypatch):
    """the reduce's tree is independent of the splits per wavefront (tests/test_gpu_parity.py
    test_gather_vpl_is_bitwise_independent_of_item_size); budget mode's reduce leaves a tile that took every call the plain run's raw sums"""
    outs = {}
    for k in (1, 2, 4):
        monkeypatch.setenv("EVPLP_GATHER_K", str(k))
        with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
            c.load_scene_json(room.jp)
            c.clear_accumulators()
            stats = []
            for i in range(2 if k != 1 else 4):
                room.iteration(evplp, c, i, splat=False)
                st = c.pass_stats(evplp.PASS_GATHER_VPL); stats.append((st["rays"], st["shaded"]))
                if i == 1:
                    outs[k] = (c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes(), stats[0], stats[1])
            if k == 1:
                plain4 = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
    monkeypatch.delenv("EVPLP_GATHER_K")
    assert outs[1][1][0] > 0 and outs[1][1][1] > 0 and np.frombuffer(outs[1][0], f32).any()
    assert outs[2] == outs[1] and outs[4] == outs[1]
    # budget mode: two warm-up calls (budgets need two folds), then budgets 0 / 1 / 2 by tile index % 3 under a window of 2, one window, a fold after every call
    budgets = (np.arange(TY * TX, dtype=np.int32) % 3).reshape(TY, TX)
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(room.jp)
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, gather_budget=True); c.adaptive_budget_window(2)
        for i in (0, 1):
            room.iteration(evplp, c, i, splat=False); c.noise_fold(1)
        c.adaptive_set_budgets(budgets)
        for i in (2, 3):
            room.iteration(evplp, c, i, splat=False); c.noise_fold(1)
        assert np.array_equal(c.adaptive_tiles(), 2 + budgets)
        acc = c.download(evplp.BUF_VPL_ACCUM)[:H]
    full = tile_mask(budgets == 2, W, H)
    assert full.any() and plain4[full].any()
    assert acc[full].tobytes() == plain4[full].tobytes()
