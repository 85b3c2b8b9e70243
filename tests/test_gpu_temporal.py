"""Temporal accumulation across the frames of a moving scene (evplp_denoise_temporal and the calls around it) on the GPU.

tests/temporal_restate.py states the previous-pose evaluation and the accumulation stage in numpy fp32, operation by operation: those are
compared bit for bit.  The a-trous passes behind the stage are test_gpu_denoise.py's restate(), fed with the restated accumulation, to the
1e-4 that file allows its spatial restatement (the last bits of exp, pow and sqrt).

The box room at 96 x 64, pt on Context(W, H, 1, 1, 1), 4 iterations per frame and one fold per iteration unless a case says otherwise; a
frame clears the accumulators, so every frame's noise estimate is its own."""
import ctypes as C
import math

import numpy as np
import pytest

import scenes
import temporal_restate as tr
from test_gpu_denoise import rel_mse, restate

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 96, 64
ITERS = 4
JITTER = (0.002, -0.001)
BOX = 3                                 # the box that moves: the largest on screen (263 pixels)
BOX_MESHES = list(range(6 + 6 * BOX, 12 + 6 * BOX))        # six room faces, then six faces per box, the light last (scenes.box_room)


def make_box(w=W, h=H):
    return scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=w / h)


@pytest.fixture(scope="module")
def box():
    return make_box()


def camera_of(box, origin=None, lookat=None):
    return tr.camera_basis(origin or box.cam_origin, lookat or box.cam_lookat, box.cam_up, box.fovy, box.aspect)


def render(evplp, c, origin, frame, iters=ITERS, jitter=None, w=W, h=H, jitter_offset=0):
    """one frame of pt: the accumulators cleared, `iters` samples with seeds of their own per frame, one fold each.  jitter = None: the
    jitter sequence from jitter_offset (the same in every frame unless the caller moves the offset)"""
    c.clear_accumulators()
    jit = evplp.jitter_sequence(jitter_offset, iters, w, h) if jitter is None else [jitter] * iters
    for i in range(iters):
        c.primary(tuple(jit[i]))
        c.path_trace(origin, 1000 * frame + i, 3, accumulate=True)
        c.noise_fold(1)


def inputs(evplp, c, s):
    return dict(rgb=c.resolve(s, s, 1.0), var=c.noise_variance(s), light=c.download(evplp.BUF_LIGHT), radius=c.scene_metrics()[0],
                guides=[c.download(b) for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG)])


def planes(evplp, c):
    return tuple(c.temporal_download(k) for k in (evplp.TEMPORAL_HISTORY_U, evplp.TEMPORAL_HISTORY_POS, evplp.TEMPORAL_HISTORY_NRM))


def expect(inp, prev, hist, cam, prev_cam, w=W, h=H, **kw):
    """the stage restated: (u_out, new history, info, filtered, albedo)"""
    pos, nrm, dif, phg = inp["guides"]
    u, filt, a = tr.pack(inp["rgb"], inp["var"], pos, nrm, dif, phg, inp["light"], h)
    sxr = F(F(0.01) * F(inp["radius"]))
    zero = np.zeros_like(pos)
    out, new, info = tr.accumulate(u, filt, pos, nrm, prev[0] if prev else zero, prev[1] if prev else zero, hist, cam, prev_cam, w, h, sxr, **kw)
    return out, new, info, filt, a


def spatial(inp, u_out, filt, a, h=H):
    """the passes on the accumulated (u, s) through test_gpu_denoise.restate: an albedo of one makes its u the given colour, and a variance
    in one channel its s (to a rounding of the division by y_r^2, far below the bar)"""
    pos, nrm, _, _ = inp["guides"]
    var = np.zeros_like(inp["rgb"]); var[..., 0] = u_out[..., 3] / (tr.Y[0] * tr.Y[0])
    one = np.ones_like(pos); zero = np.zeros_like(pos)
    den, _ = restate(u_out[..., :3], var, pos, nrm, one, zero, inp["light"], inp["radius"], h)
    return np.where(filt[..., None], a * den, inp["rgb"]).astype(F)


def same(got, want):
    return np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


def assert_stage(evplp, c, want_out, want_hist, want_info, info):
    hu, hp, hn = planes(evplp, c)
    assert same(hp, want_hist[1]) and same(hn[..., :3], want_hist[2][..., :3])
    assert same(hn[..., 3], want_hist[2][..., 3]), "history lengths"
    assert same(hu, want_out), "u_out, s_out"
    assert (info["filtered"], info["reprojected"], info["disoccluded"], info["history_sum"]) == \
        (want_info["filtered"], want_info["n_reprojected"], want_info["disoccluded"], want_info["history_sum"])
    return hu, hp, hn


def rel_err(got, want):
    floor = 1e-6 * float(np.abs(want).max())
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want.astype(np.float64)), floor)).max())


class Pose:
    """the host's copy of every mesh's vertices, moved as the device moves them"""
    def __init__(self, box):
        self.box = box
        self.rest = [m["verts"].copy() for m in box.meshes]
        self.verts = [v.copy() for v in self.rest]

    def soup(self):
        return np.concatenate([v[m["idx"]] for v, m in zip(self.verts, self.box.meshes)]).astype(F)

    def move(self, evplp, c, m, how="transform"):
        for i in BOX_MESHES:
            new = evplp.transform_points(m, self.rest[i])
            if how == "transform":
                c.transform_mesh(i, m)
            else:
                c.update_mesh(i, new)
            self.verts[i] = new
        c.refit_accel()


def box_matrix(box, angle, t):
    v = np.concatenate([box.meshes[i]["verts"] for i in BOX_MESHES])
    c = np.append((v.min(0) + v.max(0))[:2] / 2, 0.0)
    ca, sa = math.cos(angle), math.sin(angle)
    R = np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]], np.float64)
    m = np.zeros((3, 4)); m[:, :3] = R; m[:, 3] = c - R @ c + np.asarray(t, np.float64)
    return m.astype(F)


def test_the_first_call_is_evplp_denoise(evplp, box):
    s = 1.0 / ITERS
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        render(evplp, c, box.cam_origin, 0)
        inp = inputs(evplp, c, s)
        den = c.denoise(s)
        got, info = c.denoise_temporal(s)
        assert same(got, den)
        assert info["reprojected"] == 0 and info["disoccluded"] == 0 and info["frames_since_reset"] == 1
        want_out, want_hist, want_info, filt, _ = expect(inp, None, None, camera_of(box), camera_of(box))
        assert info["filtered"] == filt.sum() == info["history_sum"] and filt[:H].mean() > 0.5
        hu, hp, hn = assert_stage(evplp, c, want_out, want_hist, want_info, info)
        assert (hn[..., 3][filt] == 1).all() and (hn[..., 3][~filt] == 0).all() and (hp[..., 3] == filt).all()
        assert not c.temporal_download(evplp.TEMPORAL_PREV_POS).any()


@pytest.mark.parametrize("w, h", [(W, H), (90, 50)])
@pytest.mark.parametrize("sequence", [False, True])
def test_a_static_scene_reads_its_own_history(evplp, w, h, sequence):
    box = make_box(w, h)
    cam = camera_of(box)
    s = 1.0 / ITERS
    jitter = None if sequence else JITTER
    with evplp.Context(w, h, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        render(evplp, c, box.cam_origin, 0, jitter=jitter, w=w, h=h)
        c.denoise_temporal(s)
        hist = planes(evplp, c)
        render(evplp, c, box.cam_origin, 1, jitter=jitter, w=w, h=h)
        inp = inputs(evplp, c, s)
        got, info = c.denoise_temporal(s)
        pos, nrm = inp["guides"][:2]
        pp, pn = c.temporal_download(evplp.TEMPORAL_PREV_POS), c.temporal_download(evplp.TEMPORAL_PREV_NRM)
        surface = pos[..., 3] != 0
        surface[h:] = False
        assert surface.sum() > 0.5 * w * h
        # the walk, the jitter and the indexing are the primary pass's: the G-buffer's bits on every surface pixel
        assert same(pp[..., :3][surface], pos[..., :3][surface]) and same(pn[..., :3][surface], nrm[..., :3][surface])
        assert (pp[..., 3][surface] == 1).all()
        want_out, want_hist, want_info, filt, a = expect(inp, (pp, pn), hist, cam, cam, w, h)
        # derived, not measured: zero motion, and a pixel's own history passes every test
        assert want_info["n_reprojected"] == filt.sum() and (want_info["integral"][filt]).all() and (want_hist[2][..., 3][filt] == 2).all()
        assert info["reprojected"] == info["filtered"] == filt.sum() and info["history_sum"] == 2 * filt.sum() and info["frames_since_reset"] == 2
        assert_stage(evplp, c, want_out, want_hist, want_info, info)
        assert not same(want_out[filt], tr.pack(inp["rgb"], inp["var"], *inp["guides"], inp["light"], h)[0][filt])        # (it blended)
        want = spatial(inp, want_out, filt, a, h)
        err = rel_err(got[:h], want[:h])
        assert err < 1e-4, err
        assert same(got[~filt], inp["rgb"][~filt])


@pytest.mark.parametrize("how", ["transform", "update"])
def test_a_moved_box_is_followed_and_the_revealed_floor_starts_again(evplp, box, how):
    cam = camera_of(box)
    s = 1.0 / ITERS
    m = box_matrix(box, 0.15, (-0.9, 0.7, 0.0))
    # the motion on screen, on the host: the box's centre moves by at least six pixels
    v = np.concatenate([box.meshes[i]["verts"] for i in BOX_MESHES])
    centre = ((v.min(0) + v.max(0)) / 2).astype(F)[None]
    a0 = evplp.project_points(box.cam_origin, box.cam_lookat, box.cam_up, box.fovy, box.aspect, W, H, centre)[0]
    a1 = evplp.project_points(box.cam_origin, box.cam_lookat, box.cam_up, box.fovy, box.aspect, W, H, evplp.transform_points(m, centre))[0]
    assert math.hypot(a1[0] - a0[0], a1[1] - a0[1]) >= 6.0
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        pose = Pose(box)
        render(evplp, c, box.cam_origin, 0)
        c.denoise_temporal(s)
        hist = planes(evplp, c)
        prev_soup = pose.soup()
        pose.move(evplp, c, m, how)
        render(evplp, c, box.cam_origin, 1)
        inp = inputs(evplp, c, s)
        debug = c.temporal_download(evplp.TEMPORAL_DEBUG_HIT)
        got, info = c.denoise_temporal(s)
        pp, pn = c.temporal_download(evplp.TEMPORAL_PREV_POS), c.temporal_download(evplp.TEMPORAL_PREV_NRM)
        # the previous-pose texels: numpy's evaluation of the walk's (tri, b, g) on the previous vertices
        wp, wn = tr.prev_pose(debug, prev_soup.reshape(-1, 3, 3))
        tri = debug[..., 0].copy().view(np.int32)
        first = sum(len(mm["idx"]) for mm in box.meshes[:BOX_MESHES[0]]); count = sum(len(box.meshes[i]["idx"]) for i in BOX_MESHES)
        on_box = (tri >= first) & (tri < first + count)
        on_box[H:] = False
        assert on_box.sum() > 100
        assert same(pp[:H], wp[:H]) and same(pn[:H], wn[:H])
        assert not same(pp[..., :3][on_box], inp["guides"][0][..., :3][on_box])                    # (the box did move)
        want_out, want_hist, want_info, filt, a = expect(inp, (wp, wn), hist, cam, cam)
        # the three classes, on the host first
        rep, taps, integral = want_info["reprojected"], want_info["taps"], want_info["integral"]
        started = filt & ~rep
        moving = on_box & rep & ~integral
        assert started.sum() > 50 and (started & ~on_box).sum() > 20, "no revealed floor"
        assert moving.sum() > 50 and (moving & (taps == 4)).sum() > 20 and (moving & (taps < 4)).sum() > 10
        hu, hp, hn = assert_stage(evplp, c, want_out, want_hist, want_info, info)
        assert (hn[..., 3][started] == 1).all() and (hn[..., 3][moving] == 2).all()
        assert info["disoccluded"] == started.sum()
        err = rel_err(got[:H], spatial(inp, want_out, filt, a)[:H])
        assert err < 1e-4, err


def test_a_moved_camera(evplp, box):
    s = 1.0 / ITERS
    shift = np.array([0.0, 1.4, 0.25])
    origin2 = [float(x) for x in np.asarray(box.cam_origin) + shift]; lookat2 = [float(x) for x in np.asarray(box.cam_lookat) + shift]
    cam, cam2 = camera_of(box), camera_of(box, origin2, lookat2)
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        render(evplp, c, box.cam_origin, 0)
        c.denoise_temporal(s)
        hist = planes(evplp, c)
        c.set_camera(origin2, lookat2, box.cam_up, box.fovy, box.aspect)
        render(evplp, c, origin2, 1)
        inp = inputs(evplp, c, s)
        got, info = c.denoise_temporal(s)
        pp, pn = c.temporal_download(evplp.TEMPORAL_PREV_POS), c.temporal_download(evplp.TEMPORAL_PREV_NRM)
        pos = inp["guides"][0]
        surface = pos[..., 3] != 0
        surface[H:] = False
        assert same(pp[..., :3][surface], pos[..., :3][surface])                                  # (nothing moved but the eye)
        want_out, want_hist, want_info, filt, a = expect(inp, (pp, pn), hist, cam2, cam)
        hu, hp, hn = assert_stage(evplp, c, want_out, want_hist, want_info, info)
        # a point that lay outside the previous image has no history (by two pixels: the motion is the difference of two projections, of
        # which this frame's carries its jitter, half a pixel at most, and the taps reach one pixel)
        was, seen = tr.project(cam, W, H, pos[..., :3])
        outside = filt & (~seen | (was[..., 0] <= -3) | (was[..., 0] >= W + 2) | (was[..., 1] <= -3) | (was[..., 1] >= H + 2))
        assert outside.sum() > 50 and (hn[..., 3][outside] == 1).all()
        assert want_info["n_reprojected"] > 1000 and (~want_info["integral"][want_info["reprojected"]]).any()
        err = rel_err(got[:H], spatial(inp, want_out, filt, a)[:H])
        assert err < 1e-4, err


def test_the_history_length_stops_at_max_history(evplp, box):
    s = 1.0 / 2
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        lengths = []
        for f in range(5):
            render(evplp, c, box.cam_origin, f, iters=2)
            _, info = c.denoise_temporal(s, max_history=3)
            hn = c.temporal_download(evplp.TEMPORAL_HISTORY_NRM)[..., 3]
            filt = c.temporal_download(evplp.TEMPORAL_HISTORY_POS)[..., 3] != 0
            assert len(np.unique(hn[filt])) == 1 and info["history_sum"] == int(hn[filt][0]) * filt.sum()
            lengths.append(int(hn[filt][0]))
        assert lengths == [1, 2, 3, 3, 3]


def test_a_reset_and_a_new_triangle_count_start_again(evplp, box):
    s = 1.0 / 2
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        for f in range(2):
            render(evplp, c, box.cam_origin, f, iters=2)
            _, info = c.denoise_temporal(s)
        assert info["frames_since_reset"] == 2 and info["reprojected"] == info["filtered"]
        c.temporal_reset()
        render(evplp, c, box.cam_origin, 2, iters=2)
        den = c.denoise(s)
        got, info = c.denoise_temporal(s)
        assert same(got, den) and info["reprojected"] == 0 and info["frames_since_reset"] == 1
        render(evplp, c, box.cam_origin, 3, iters=2)
        _, info = c.denoise_temporal(s)
        assert info["frames_since_reset"] == 2 and info["reprojected"] == info["filtered"]
        # one more triangle in the scene: the previous pose describes another scene
        mat = c.add_material((0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 1.0)
        c.add_mesh(np.array([[4.0, 4.0, 0.5], [4.5, 4.0, 0.5], [4.0, 4.5, 0.5]], F), np.array([[0, 1, 2]], np.int32), mat)
        c.build_accel()
        with pytest.raises(evplp.EvplpError) as e:
            c.denoise_temporal(s)                                  # (no primary pass since the build)
        assert e.value.status == evplp.ERR_INVALID
        render(evplp, c, box.cam_origin, 4, iters=2)
        den = c.denoise(s)
        got, info = c.denoise_temporal(s)
        assert same(got, den) and info["reprojected"] == 0 and info["frames_since_reset"] == 1


def _refused(evplp, fn, needle=None):
    with pytest.raises(evplp.EvplpError) as e:
        fn()
    assert e.value.status == evplp.ERR_INVALID, str(e.value)
    if needle:
        assert needle in str(e.value), str(e.value)


def test_a_refused_call_changes_nothing(evplp, box):
    s = 1.0 / 2

    def sequence(refuse):
        with evplp.Context(W, H, 1, 1, 1) as c:
            box.upload(c); c.noise_track(True); c.temporal_enable(True)
            render(evplp, c, box.cam_origin, 0, iters=2)
            c.denoise_temporal(s)
            if refuse:
                for kw in (dict(max_history=1025), dict(max_history=-1), dict(normal_cos=1.5), dict(normal_cos=-0.1), dict(normal_cos=float("nan")),
                           dict(levels=11), dict(sigma_position=-1.0)):
                    _refused(evplp, lambda: c.denoise_temporal(s, **kw))
                p, t = evplp.DenoiseParams(), evplp.TemporalParams()
                assert evplp.lib().evplp_denoise_temporal(c._h, s, 1.0, 0, C.byref(p), C.byref(t), None, None) == evplp.ERR_INVALID      # a null output
                c.upload(evplp.BUF_GBUF_POSITION, c.download(evplp.BUF_GBUF_POSITION))
                _refused(evplp, lambda: c.denoise_temporal(s), "evplp_primary")                 # the position plane is the caller's upload
            render(evplp, c, box.cam_origin, 1, iters=2)
            if refuse:
                c.noise_track(False)
                _refused(evplp, lambda: c.denoise_temporal(s), "tracking")
                c.noise_track(True)
                render(evplp, c, box.cam_origin, 1, iters=2)
            got, info = c.denoise_temporal(s)
            return got, planes(evplp, c), info
    plain, refused = sequence(False), sequence(True)
    assert same(plain[0], refused[0]) and all(same(a, b) for a, b in zip(plain[1], refused[1])) and plain[2] == refused[2]
    assert plain[2]["frames_since_reset"] == 2 and plain[2]["reprojected"] == plain[2]["filtered"]
    # the refusals that need a state of their own
    with evplp.Context(W, H, 1, 1, 1) as c:
        _refused(evplp, lambda: c.denoise_temporal(s))                                          # no scene
        box.upload(c); c.noise_track(True)
        render(evplp, c, box.cam_origin, 0, iters=2)
        _refused(evplp, lambda: c.denoise_temporal(s), "evplp_temporal_enable")                 # not enabled
        _refused(evplp, lambda: c.temporal_reset(), "evplp_temporal_enable")
        c.temporal_enable(True)
        render(evplp, c, box.cam_origin, 0, iters=1)
        _refused(evplp, lambda: c.denoise_temporal(1.0), "fold")                                # one closed batch
        render(evplp, c, box.cam_origin, 0, iters=2)
        c.update_mesh(BOX_MESHES[0], box.meshes[BOX_MESHES[0]]["verts"])
        _refused(evplp, lambda: c.denoise_temporal(s), "evplp_refit_accel")                     # a dirty scene
        c.refit_accel()
        _refused(evplp, lambda: c.denoise_temporal(s), "evplp_primary")                         # no primary pass since the refit
        render(evplp, c, box.cam_origin, 0, iters=2)
        got, info = c.denoise_temporal(s)
        assert np.isfinite(got).all() and info["frames_since_reset"] == 1
    with evplp.Context(W, H, 1, 1, 1, strip_rank=0, strip_count=2, strip_rows=16) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        render(evplp, c, box.cam_origin, 0, iters=2)
        _refused(evplp, lambda: c.denoise_temporal(s), "evplp_group_denoise_temporal")          # a row-strip context
        assert np.isfinite(c.resolve(s, s, 1.0)).all()


def test_a_context_that_never_enables_it_allocates_nothing(evplp, box):
    """Device memory in use around evplp_denoise_temporal's own arrays on a large image: a context that only ever calls evplp_denoise grows by
    nothing when the feature exists; enabling it adds 32 B per plane pixel (and 36 B per triangle), the first call 96 B per pixel -- which
    shows that the figure would see them."""
    import torch
    w, h = 1280, 720
    big = make_box(w, h)
    px = w * h

    def in_use():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free
    with evplp.Context(w, h, 1, 1, 1) as c:
        big.upload(c); c.noise_track(True)
        render(evplp, c, big.cam_origin, 0, iters=2, w=w, h=h)
        c.denoise(0.5); c.synchronize()
        m0 = in_use()
        render(evplp, c, big.cam_origin, 1, iters=2, w=w, h=h)
        c.denoise(0.5); c.synchronize()
        assert abs(in_use() - m0) <= (2 << 20)
        c.temporal_enable(True); c.synchronize()
        m1 = in_use()
        rows = c.local_rows
        assert 32 * w * rows <= m1 - m0 <= 32 * w * rows + (8 << 20), (m1 - m0, 32 * w * rows)
        c.denoise_temporal(0.5); c.synchronize()
        m2 = in_use()
        assert 96 * w * rows <= m2 - m1 <= 96 * w * rows + (8 << 20), (m2 - m1, 96 * w * rows)
        c.temporal_enable(False); c.synchronize()
        assert in_use() <= m0 + (2 << 20)


def test_gain_over_the_spatial_filter_on_a_moving_sequence(evplp, box):
    """Eight frames, the box moving a little in each, pt at 2 iterations per frame with seeds and jitters of their own per frame; relMSE of the
    last frame against 512 iterations of its pose (other seeds).  The bar is the parent's filter measured here, on the same last frame.
    Measured on one MI355X: raw 0.22720, evplp_denoise 0.02304, evplp_denoise_temporal 0.01066 -- ratio 0.463 at a mean history length of 7.55
    (DESIGN section 6b).  The bar stays the spatial filter's own figure."""
    frames, iters = 8, 2
    s = 1.0 / iters
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        pose = Pose(box)
        for f in range(frames):
            if f:
                pose.move(evplp, c, box_matrix(box, 0.02 * f, (-0.12 * f, 0.09 * f, 0.0)))
            render(evplp, c, box.cam_origin, f, iters=iters, jitter_offset=iters * f)
            if f == frames - 1:
                spatial_only = c.denoise(s)[:H]
                raw = c.resolve(s, s, 1.0)[:H]
            got, info = c.denoise_temporal(s)
        assert info["frames_since_reset"] == frames and info["reprojected"] > 0.9 * info["filtered"]
        c.temporal_enable(False); c.noise_track(False)
        c.clear_accumulators()
        jit = evplp.jitter_sequence(10000, 512, W, H)
        for i in range(512):
            c.primary(tuple(jit[i])); c.path_trace(box.cam_origin, 50000 + i, 3, accumulate=True)
        ref = c.resolve(1.0 / 512, 1.0 / 512, 1.0)[:H]
    e_raw, e_sp, e_tp = rel_mse(raw, ref), rel_mse(spatial_only, ref), rel_mse(got[:H], ref)
    print(f"\nrelMSE of frame {frames - 1}: raw {e_raw:.5f}, evplp_denoise {e_sp:.5f}, evplp_denoise_temporal {e_tp:.5f}, ratio {e_tp / e_sp:.3f}; "
          f"mean history {info['history_sum'] / info['filtered']:.2f}")
    assert e_tp <= e_sp, (e_tp, e_sp)


def _sequence(evplp, runner, box, frames=3, rebalance_at=None):
    """a moving sequence of pt frames on a context or a group: (image, history planes) of every frame"""
    group = isinstance(runner, evplp.Group)
    out = []
    for f in range(frames):
        if f:
            m = box_matrix(box, 0.05 * f, (-0.3 * f, 0.25 * f, 0.0))
            for i in BOX_MESHES:
                runner.transform_mesh(i, m)
            runner.refit_accel()
        if group and rebalance_at == f:
            _deal(evplp, runner, box)
        runner.clear_accumulators()
        jit = evplp.jitter_sequence(2 * f, 2, W, H)
        for i in range(2):
            runner.primary(tuple(jit[i]))
            runner.path_trace(box.cam_origin, 1000 * f + i, 3, accumulate=True)
            runner.noise_fold(1)
        img, info = runner.denoise_temporal(0.5)
        out.append((img[:H], tuple(runner.temporal_download(k)[:H] for k in range(3)), info))
    return out


def test_partitions(evplp, box):
    with evplp.Context(W, H, 1, 1, 1) as c:
        box.upload(c); c.noise_track(True); c.temporal_enable(True)
        one = _sequence(evplp, c, box)
    assert one[2][2]["reprojected"] > 0 and one[2][2]["disoccluded"] > 0
    for n in (2, 3):
        for dealt in (False, True):
            with evplp.Group(W, H, GNL, GNV, GP, n, devices=[0] * n, deterministic=True) as g:
                _upload_group(evplp, g, box)
                g.noise_track(True); g.temporal_enable(True)
                if dealt:            # a deal by measured cost, then another between frames 1 and 2: the history stays in image layout
                    _deal(evplp, g, box)
                    assert len(set(g.block_owners().tolist())) == n
                got = _sequence(evplp, g, box, rebalance_at=2 if dealt else None)
                for f in range(3):
                    assert same(got[f][0], one[f][0]), (n, dealt, f)
                    assert all(same(a, b) for a, b in zip(got[f][1], one[f][1])), (n, dealt, f, "history")
                    assert got[f][2] == one[f][2], (n, dealt, f)
    with evplp.Group(W, H, 1, 1, 1, 3, devices=[0] * 3, partition="iterations") as g:
        _upload_group(evplp, g, box)
        g.noise_track(True); g.temporal_enable(True)
        got = []
        for f in range(3):
            if f:
                m = box_matrix(box, 0.05 * f, (-0.3 * f, 0.25 * f, 0.0))
                for i in BOX_MESHES:
                    g.transform_mesh(i, m)
                g.refit_accel()
            g.clear_accumulators()
            jit = evplp.jitter_sequence(2 * f, 2, W, H)
            for i in range(2):
                g.select_rank((2 * f + i) % 3)
                g.primary(tuple(jit[i])); g.path_trace(box.cam_origin, 1000 * f + i, 3, accumulate=True); g.noise_fold(1)
            img, info = g.denoise_temporal(0.5)
            got.append((img, info))
        # (the ranks' sums are added in rank order and their moments pooled: test_gpu_denoise's test_partitions allows its restatement 1e-4
        # there for the same reason; the counts of the stage are the single context's wherever no threshold sits within that of a tap)
        for f in range(3):
            assert rel_err(got[f][0], one[f][0]) < 1e-4, f
            assert got[f][1]["filtered"] == one[f][2]["filtered"] and got[f][1]["frames_since_reset"] == f + 1


GNL, GNV, GP = 512, 16, 2             # light paths of the calibration frame alone (a deal by cost needs a gather to clock)


def _deal(evplp, g, box):
    bsr = g.rank(0).scene_metrics()[0]
    r = 0.05 * bsr
    fp = evplp.frame_params(camera_pos=box.cam_origin, mis_mode="balance", pdf_mc=(GNV / GNL) / math.pi / (r * r), photon_radius=r, num_light_paths=GNL,
                            num_vpl_light_paths=GNV, photons_per_path=GP, do_accumulate=1, rng_seed=0, jitter=JITTER)
    g.calibrate(True)
    g.primary(JITTER); g.trace_light_paths(0); g.gather(fp, 0)
    g.rebalance()


def _upload_group(evplp, g, box):
    for r in range(g.n):
        box.upload(g.rank(r))


def test_json_temporal_and_rng_advance(evplp, tmp_path):
    """The technique JSON on test_gpu_transform's animated room, pt: with "temporal" every frame's denoised file is the API sequence's image
    and frame 0's is the file of the run without the key; the stat keys appear only with it; with "rngAdvance": k frame f's raw output is a
    fresh render of the moved scene at rngOffset + f k."""
    import json
    from test_gpu_transform import H as TH, W as TW, _anim_matrices, _scene_dir
    frames, k, rng = 3, 5, 3
    mats = [_anim_matrices(f) for f in range(frames)]
    anim = {"frames": frames, "rngAdvance": k, "tracks": [{"object": 1, "matrices": [m[0] for m in mats]}, {"mesh": 0, "matrices": [m[1] for m in mats]}]}
    noise = {"filename": "n.json", "batchIterations": 1}
    d0 = _scene_dir(evplp, tmp_path, "plain", "pt")
    evplp.render_json(str(d0 / "room.json"), json.dumps({"animation": anim, "noise": noise, "denoise": {"filename": "d.pfm"}}))
    d1 = _scene_dir(evplp, tmp_path, "temporal", "pt")
    evplp.render_json(str(d1 / "room.json"), json.dumps({"animation": anim, "noise": noise, "denoise": {"filename": "d.pfm", "temporal": {"maxHistory": 8}}}))
    assert (d1 / "d_f0000.pfm").read_bytes() == (d0 / "d_f0000.pfm").read_bytes()
    assert (d1 / "d_f0002.pfm").read_bytes() != (d0 / "d_f0002.pfm").read_bytes()
    for f in range(frames):
        assert (d1 / f"pt_f{f:04d}.pfm").read_bytes() == (d0 / f"pt_f{f:04d}.pfm").read_bytes()          # (the raw outputs do not change)
        st0, st1 = json.load(open(d0 / f"pt_f{f:04d}.json")), json.load(open(d1 / f"pt_f{f:04d}.json"))
        keys = {"temporalReprojected", "temporalDisoccluded", "temporalMeanHistory"}
        assert not keys & set(st0) and keys <= set(st1), (st0, st1)
        assert (st1["temporalReprojected"] > 0) == (f > 0) and 1.0 <= st1["temporalMeanHistory"] <= f + 1
        # rngAdvance: a fresh render of the moved scene at rngOffset + f k
        dr = _scene_dir(evplp, tmp_path, f"fresh{f}", "pt", move=mats[f])
        evplp.render_json(str(dr / "room.json"), json.dumps({"rngOffset": rng + f * k}))
        assert (dr / "pt.pfm").read_bytes() == (d0 / f"pt_f{f:04d}.pfm").read_bytes(), f
    # the API sequence: the same frames through a context
    sd, _ = scenes.load_obj_scene(str(d1 / "room.json"))
    extra = len(sd.meshes) - 2                                                # (the objects' meshes in order, the light last)
    with evplp.Context(TW, TH, 1, 1, 1) as c:
        c.load_scene_json(str(d1 / "room.json")); c.noise_track(True); c.temporal_enable(True)
        for f in range(frames):
            c.transform_mesh(extra, mats[f][0]); c.transform_mesh(0, mats[f][1]); c.refit_accel()
            c.clear_accumulators()
            jit = evplp.jitter_sequence(rng + f * k, 2, TW, TH)
            for i in range(2):
                c.primary(tuple(jit[i])); c.path_trace(sd.cam_origin, rng + f * k + i, 3, accumulate=True); c.noise_fold(1)
            img, _ = c.denoise_temporal(0.5, max_history=8)
            assert np.array_equal(np.flipud(img[:TH]), evplp.load_pfm(str(d1 / f"d_f{f:04d}.pfm"))), f
