"""Per-pixel noise from the running sums, without a reference image (evplp_noise_*, evplp_group_noise_* and the technique JSON's "noise"
block), on the 96 x 64 room of tests/test_gpu_convergence.py.

Q, S, the variance image and the three figures are recomputed in numpy from the accumulators downloaded after every iteration (the variance
image bit for bit, the figures to 1e-12); one context, row strips round robin and dealt by cost give the same doubles; the iteration
partition pools its shards to the same figures within 1e-5; the overlapped light tracing and a photon splat re-run after a bins overflow
change nothing; on the path tracer the estimate predicts the squared difference of two independent runs; and in the technique loops the
block writes its checkpoints and variance image without touching the written images."""
import json

import numpy as np
import pytest

import scenes
from test_gpu_convergence import NL, NV, P, H, W, close, params, reference_and_mask, render, room

pytestmark = pytest.mark.gpu

ITERS = 12
SCHEDULES = ([1] * 12, [3] * 4, [2, 4, 2, 4])


@pytest.fixture(scope="module")
def scene(evplp, tmp_path_factory):
    d = tmp_path_factory.mktemp("noise_scene")
    jp = room(evplp, d)
    sd, _ = scenes.load_obj_scene(jp)
    return jp, sd


def one_iteration(runner, fp, i, group):
    runner.primary((0.002, -0.001)); runner.trace_light_paths(i)
    if group:
        runner.gather(fp, 0)
    else:
        runner.gather_vpl(fp)
    runner.splat_photons(fp)


def sums(evplp, c):
    """c = rgb(VPL) + rgb(photon), fp32, over the context's local rows"""
    return (c.download(evplp.BUF_VPL_ACCUM)[..., :3] + c.download(evplp.BUF_PHOTON_ACCUM)[..., :3]).astype(np.float32)


def numpy_variance(cs, schedule, scale, with_v=False):
    """cs[j]: the sums after j iterations (cs[0] where tracking started; only the fold boundaries are read, so a dict will do); the variance
    image of scale * c (fp64).  A NaN v reads 0 and an infinite one stays, as in the library.  with_v: also v = (Q - S^2 / K) / (B - 1) before
    the clamp, which numpy_figures wants for the rule on broken pixels."""
    prev = cs[0]; q = np.zeros(prev.shape, np.float64); it = 0
    for k in schedule:
        it += k
        d = (cs[it] - prev).astype(np.float32).astype(np.float64)
        q = q + d * d / np.float64(k)
        prev = cs[it]
    K, B = float(sum(schedule)), float(len(schedule))
    s = (prev - cs[0]).astype(np.float32).astype(np.float64)
    v = (q - s * s / K) / (B - 1.0)
    s2K = np.float64(np.float32(scale)) ** 2 * K                 # (the library takes the scale as a float)
    var = s2K * np.where(v > 0.0, v, 0.0)
    return (var, v) if with_v else var


def broken_pixels(v, den, emitter):
    """include/evplp.h, "non-finite sums": a pixel is broken when its den is not finite or any of its three v is not (v = None: the caller
    vouches for finite moments); a pixel that mask_emitter hides reads no moments, so only its den can break it"""
    broken = ~np.isfinite(den)
    if v is not None:
        broken = broken | (~np.isfinite(v).all(-1) & ~emitter)
    return broken


def numpy_figures(var, composite, light, ls, mask_emitter, mask_top_down=None, v=None):
    """var (H, W, 3) fp64 and composite (H, W, 3) fp32 as resolve() returns it (y = 0 at the bottom); v: numpy_variance(.., with_v=True)'s.
    A broken pixel's num and rel are NaN: an image figure says that it is broken."""
    num = (var[..., 0] + var[..., 1]) + var[..., 2]
    emitter = np.zeros(num.shape, bool)
    if mask_emitter:
        emitter = np.float32(0.0) < light[..., 0] * np.float32(ls)
        num = np.where(emitter, 0.0, num)
    cp = composite.astype(np.float64)
    den = ((cp[..., 0] * cp[..., 0] + cp[..., 1] * cp[..., 1]) + cp[..., 2] * cp[..., 2]) + 0.001
    num = np.where(broken_pixels(v, den, emitter), np.nan, num)
    rel = num / den
    keep = np.ones(num.shape, bool) if mask_top_down is None else mask_top_down[::-1].any(-1)
    kept = int(keep.sum())
    return num.sum() / num.size, rel.sum() / num.size, (rel[keep].sum() / kept if kept else 0.0)


def run_context(evplp, jp, sd, schedule, **ctx_kw):
    """12 iterations, folded by `schedule`; returns the sums after every iteration and the device's figures / variance at scale 1/12"""
    with evplp.Context(W, H, NL, NV, P, deterministic=True, **ctx_kw) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        c.clear_accumulators()
        c.noise_track(True, reference_and_mask())
        cs = [sums(evplp, c)]
        bounds = set(np.cumsum(schedule).tolist())
        it = 0; last = 0
        for i in range(ITERS):
            one_iteration(c, params(evplp, sd, bsr, total, i), i, False)
            it += 1
            cs.append(sums(evplp, c))
            if it in bounds:
                c.noise_fold(it - last); last = it
        s = 1.0 / ITERS
        out = dict(cs=cs, est=c.noise_estimate(s), est_me=c.noise_estimate(s, 1.0, mask_emitter=True), var=c.noise_variance(s)[:H],
                   composite=c.resolve(s, s, 1.0)[:H], composite_me=c.resolve(s, s, 1.0, mask_emitter=True)[:H],
                   light=c.download(evplp.BUF_LIGHT)[:H])
    return out


def test_exact_against_numpy_for_every_batch_schedule(evplp, scene):
    jp, sd = scene
    mask = reference_and_mask()
    s = 1.0 / ITERS
    for schedule in SCHEDULES:
        r = run_context(evplp, jp, sd, schedule)
        var = numpy_variance([x[:H] for x in r["cs"]], schedule, s)
        assert var.max() > 0
        assert r["var"].tobytes() == var.astype(np.float32).tobytes(), schedule          # the variance image bit for bit
        close(r["est"], numpy_figures(var, r["composite"], r["light"], 1.0, False, mask), 1e-12)
        close(r["est_me"], numpy_figures(var, r["composite_me"], r["light"], 1.0, True, mask), 1e-12)
        assert r["est_me"][0] <= r["est"][0]


def test_refusals_and_restart(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        with pytest.raises(evplp.EvplpError):
            c.noise_fold(1)                                       # tracking off
        with pytest.raises(evplp.EvplpError):
            c.noise_estimate(1.0)
        c.clear_accumulators()
        c.noise_track(True)
        with pytest.raises(evplp.EvplpError):
            c.noise_estimate(1.0)                                 # B = 0
        one_iteration(c, params(evplp, sd, bsr, total, 0), 0, False); c.noise_fold(1)
        with pytest.raises(evplp.EvplpError) as e:
            c.noise_estimate(1.0)                                 # B = 1
        assert ">= 2" in str(e.value)
        with pytest.raises(evplp.EvplpError):
            c.noise_variance(1.0)
        # tracking started mid-run: the moments cover the folds after the snapshot only
        cs = [sums(evplp, c)]
        c.noise_track(True)
        for i in (1, 2, 3):
            one_iteration(c, params(evplp, sd, bsr, total, i), i, False); c.noise_fold(1); cs.append(sums(evplp, c))
        assert c.noise_variance(0.25)[:H].tobytes() == numpy_variance([x[:H] for x in cs], [1, 1, 1], 0.25).astype(np.float32).tobytes()
        # a clear starts again from the empty sums
        c.clear_accumulators()
        one_iteration(c, params(evplp, sd, bsr, total, 4), 4, False); c.noise_fold(1)
        with pytest.raises(evplp.EvplpError):
            c.noise_estimate(1.0)
        c.noise_track(False)
        with pytest.raises(evplp.EvplpError):
            c.noise_fold(1)


def test_partitions_give_the_same_figures(evplp, scene):
    jp, sd = scene
    mask = reference_and_mask()
    s = 1.0 / ITERS
    one = run_context(evplp, jp, sd, [1] * ITERS)
    with evplp.Context(W, H, NL, NV, P) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
    with evplp.Group(W, H, NL, NV, P, 3, devices=[0] * 3, deterministic=True) as g:
        g.load_scene_json(jp)
        with pytest.raises(evplp.EvplpError):
            g.noise_fold(1)                                       # refused on the caller's thread; the group stays usable
        fp_of = lambda i: params(evplp, sd, bsr, total, i)
        for dealt in (False, True):
            if dealt:
                g.calibrate(True)
                one_iteration(g, fp_of(0), 0, True)
                g.rebalance()
            g.clear_accumulators()
            g.noise_track(True, mask)
            for i in range(ITERS):
                one_iteration(g, fp_of(i), i, True)
                g.noise_fold(1)
            assert g.noise_estimate(s) == one["est"], dealt
            assert g.noise_estimate(s, 1.0, mask_emitter=True) == one["est_me"], dealt
            assert g.noise_variance(s).tobytes() == one["var"].tobytes(), dealt
    with evplp.Group(W, H, NL, NV, P, 3, devices=[0] * 3, deterministic=True, partition="iterations") as g:
        g.load_scene_json(jp)
        g.clear_accumulators()
        g.noise_track(True, mask)
        for i in range(ITERS):
            g.select_rank(i % 3)
            one_iteration(g, fp_of(i), i, True)
            g.noise_fold(1)
        got = g.noise_estimate(s)
        close(got, one["est"], 1e-5)
        close(g.noise_estimate(s, 1.0, mask_emitter=True), one["est_me"], 1e-5)
        var = g.noise_variance(s).astype(np.float64)
        ref = one["var"].astype(np.float64)
        assert np.sqrt(((var - ref) ** 2).sum() / (ref ** 2).sum()) < 1e-5


def test_overlap_and_a_splat_rerun_change_nothing(evplp, scene, monkeypatch):
    jp, sd = scene
    base = run_context(evplp, jp, sd, [2] * 6)
    over = run_context(evplp, jp, sd, [2] * 6, overlap_light_tracing=True)
    assert over["est"] == base["est"] and over["var"].tobytes() == base["var"].tobytes()
    monkeypatch.setenv("EVPLP_BIN_STRIDE", "2")                   # every splat overflows its bins and runs again (settle_splat)
    rerun = run_context(evplp, jp, sd, [2] * 6, overlap_light_tracing=True)
    monkeypatch.delenv("EVPLP_BIN_STRIDE")
    assert rerun["est"] == base["est"] and rerun["var"].tobytes() == base["var"].tobytes()


def test_calibration_on_the_path_tracer(evplp, scene):
    """Two path-traced runs of 32 iterations with disjoint seeds: mean_p |img_A - img_B|^2 against mse_A + mse_B.
    Observed on one MI355X: mean |A - B|^2 = 0.00483 against mse_A + mse_B = 0.00472, ratio 1.024."""
    jp, _ = scene
    n = 32
    sd, _ = scenes.load_obj_scene(jp)

    def run(offset):
        with evplp.Context(W, H, 1, 1, 1) as c:
            c.load_scene_json(jp)
            jit = evplp.jitter_sequence(offset, n, W, H)
            c.clear_accumulators()
            c.noise_track(True)
            for i in range(n):
                c.primary(tuple(jit[i]))
                c.path_trace(sd.cam_origin, offset + i, 3, accumulate=True)
                c.noise_fold(1)
            return c.resolve(1.0 / n, 0.0, 0.0)[:H].astype(np.float64), c.noise_estimate(1.0 / n, 0.0)

    a, ea = run(0)
    b, eb = run(100000)
    diff = ((a - b) ** 2).sum(-1).mean()
    ratio = diff / (ea[0] + eb[0])
    print(f"calibration: mean |A - B|^2 = {diff:.6g}, mse_A + mse_B = {ea[0] + eb[0]:.6g}, ratio {ratio:.4f}")
    assert 0.8 <= ratio <= 1.2, (ratio, diff, ea[0], eb[0])


NOISE = {"everyIterations": 2, "filename": "noise.json", "varianceFilename": "var.pfm"}


def render_noise(evplp, d, jp, technique, block=None, **extra):
    if block is not None:
        extra = dict(extra, noise=block)
    imgs, st, _ = render(evplp, d, jp, technique, None, **extra)
    curve = json.load(open(d / "noise.json")) if block is not None else None
    return imgs, st, curve


@pytest.mark.parametrize("technique, device", [("photonfam", None), ("pt", None), ("photonfam", dict(gpus=3, virtual=True, partition="iterations"))])
def test_technique_loop_checkpoints_variance_and_unchanged_outputs(evplp, scene, tmp_path, technique, device):
    jp, _ = scene
    extra = {} if device is None else {"device": device}
    plain, st_plain, _ = render_noise(evplp, tmp_path / "plain", jp, technique, **extra)
    imgs, st, curve = render_noise(evplp, tmp_path / "noise", jp, technique, NOISE, **extra)
    assert imgs == plain                                                 # byte-identical images
    assert st["numIterations"] == st_plain["numIterations"] == 7 and sorted(st) == sorted(st_plain)
    cps = curve["checkpoints"]
    if device is None:
        assert [p["iteration"] for p in cps] == [2, 4, 6, 7] and [p["batches"] for p in cps] == [2, 4, 6, 7]
    else:
        assert cps[-1]["iteration"] == 7 and cps[-1]["batches"] == 7
    assert all(a["timeMs"] <= b["timeMs"] for a, b in zip(cps, cps[1:]))
    assert curve["pixels"] == W * H and curve["batchIterations"] == 1 and all(p["relMse"] > 0 for p in cps)
    # the variance file is the variance of the saved image: its mean over pixels of the channel sum is the last checkpoint's mse
    var = evplp.load_pfm(str(tmp_path / "noise" / "var.pfm")).astype(np.float64)
    assert var.shape == (H, W, 3) and var.min() >= 0
    assert abs(var.sum(-1).mean() - cps[-1]["mse"]) <= 1e-6 * cps[-1]["mse"]


def test_variance_file_is_noise_variance_flipped(evplp, scene, tmp_path):
    """The pt loop driven by hand on one context (jitter, seeds, accumulation as rtpt2.h) against the file the technique writes."""
    jp, _ = scene
    imgs, st, curve = render_noise(evplp, tmp_path / "noise", jp, "pt", dict(NOISE, batchIterations=1))
    sd, _ = scenes.load_obj_scene(jp)
    n = 7
    with evplp.Context(W, H, 1, 1, 1) as c:
        c.load_scene_json(jp)
        jit = evplp.jitter_sequence(0, n, W, H)
        c.clear_accumulators()
        c.noise_track(True)
        for i in range(n):
            c.primary(tuple(jit[i]))
            c.path_trace(sd.cam_origin, i, 3, accumulate=True)
            c.noise_fold(1)
        var = c.noise_variance(1.0 / n)[:H]
        est = c.noise_estimate(1.0 / n)
    got = evplp.load_pfm(str(tmp_path / "noise" / "var.pfm"))
    assert got.tobytes() == np.ascontiguousarray(var[::-1]).tobytes()
    last = curve["checkpoints"][-1]
    assert (last["mse"], last["relMse"]) == (est[0], est[1])


def test_stop_rel_mse_ends_the_run_at_its_checkpoint(evplp, scene, tmp_path):
    jp, _ = scene
    _, _, first = render_noise(evplp, tmp_path / "first", jp, "photonfam", NOISE)
    cps = first["checkpoints"]
    stop = [p for p in cps if p["iteration"] == 4][0]["relMse"] + 1e-12
    at = min(p["iteration"] for p in cps if p["relMse"] <= stop)
    assert at <= 4
    _, st, second = render_noise(evplp, tmp_path / "second", jp, "photonfam", dict(NOISE, stopRelMse=stop))
    assert [p["iteration"] for p in second["checkpoints"]] == [i for i in (2, 4) if i <= at]
    assert second["checkpoints"][-1]["iteration"] == at == st["numIterations"]
    for a, b in zip(cps, second["checkpoints"]):
        assert (a["mse"], a["relMse"]) == (b["mse"], b["relMse"])
