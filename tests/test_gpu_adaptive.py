"""Adaptive gather (evplp_adaptive_*, evplp_group_adaptive_* and the technique JSON's "adaptive" block) on the 96 x 64 room of
tests/test_gpu_convergence.py.

A plain run and an adaptive run of the same iterations are compared: active tiles and the photon accumulator bit for bit, retired pixels
against numpy's extrapolation of the plain run's accumulator, the set of retired tiles against numpy's restatement of the criterion, the
frozen variance of retired pixels bit for bit; fewer shadow rays once tiles retire and none when all have; row strips of 2 and 3 virtual
ranks, round robin and dealt by cost, against one context; a VSL run; every refusal; and the technique loop's block."""
import json
import math

import numpy as np
import pytest

import scenes
from test_gpu_convergence import NL, NV, P, H, W, params, room, write_inputs
from test_gpu_noise import broken_pixels

pytestmark = pytest.mark.gpu

ITERS, RETIRE_AT, MIN_BATCHES = 12, 4, 3
TX, TY = (W + 7) // 8, (H + 7) // 8


@pytest.fixture(scope="module")
def scene(evplp, tmp_path_factory):
    d = tmp_path_factory.mktemp("adaptive_scene")
    jp = room(evplp, d)
    sd, _ = scenes.load_obj_scene(jp)
    return jp, sd


def vsl_params(evplp, sd, bsr, total, i):
    fp = params(evplp, sd, bsr, total, i)
    r = 0.05 * bsr
    fp.vsl_radius = r; fp.vsl_inv_pi_radius2 = 1.0 / (math.pi * r * r)
    return fp


def one_iteration(runner, fp, i, group, vsl=False):
    runner.primary((0.002, -0.001)); runner.trace_light_paths(i)
    if group:
        runner.gather(fp, 1 if vsl else 0)
    elif vsl:
        runner.gather_vsl(fp)
    else:
        runner.gather_vpl(fp)
    runner.splat_photons(fp)


def sums(evplp, c):
    return (c.download(evplp.BUF_VPL_ACCUM)[..., :3] + c.download(evplp.BUF_PHOTON_ACCUM)[..., :3]).astype(np.float32)[:H]


def moments(cs):
    """cs[j]: the sums after j iterations, one fold per iteration: per pixel and channel (Q - S^2 / K) / (B - 1), fp64, and K = B"""
    q = np.zeros(cs[0].shape, np.float64)
    for j in range(1, len(cs)):
        d = (cs[j] - cs[j - 1]).astype(np.float32).astype(np.float64)
        q = q + d * d / np.float64(1.0)
    K = float(len(cs) - 1)
    s = (cs[-1] - cs[0]).astype(np.float32).astype(np.float64)
    return (q - s * s / K) / (K - 1.0), K


def variance(v, s2K):
    return s2K * np.where(v > 0.0, v, 0.0)


def rel_of(var, composite, light, ls=1.0, mask_emitter=False, v=None):
    """num and rel per pixel; a broken pixel's are NaN (test_gpu_noise.broken_pixels; v: the moments before the clamp, None = finite)"""
    num = (var[..., 0] + var[..., 1]) + var[..., 2]
    emitter = np.zeros(num.shape, bool)
    if mask_emitter:
        emitter = np.float32(0.0) < light[..., 0] * np.float32(ls)
        num = np.where(emitter, 0.0, num)
    cp = composite.astype(np.float64)
    den = ((cp[..., 0] * cp[..., 0] + cp[..., 1] * cp[..., 1]) + cp[..., 2] * cp[..., 2]) + 0.001
    num = np.where(broken_pixels(v, den, emitter), np.nan, num)
    return num, num / den


def tile_means(rel, w=W, h=H):
    """the retire kernel's per-tile mean: lane = (y % 8) * 8 + x % 8, a shuffle-down tree over the 64 lanes, / the tile's sound in-image
    pixels.  A broken pixel (rel_of: a NaN rel) adds nothing and is not counted; a tile without a sound pixel reads 0."""
    ty_n, tx_n = (h + 7) // 8, (w + 7) // 8
    out = np.zeros((ty_n, tx_n), np.float64)
    for ty in range(ty_n):
        for tx in range(tx_n):
            lanes = np.zeros(64, np.float64); cnt = np.zeros(64, np.float64)
            for ly in range(8):
                for lx in range(8):
                    y, x = ty * 8 + ly, tx * 8 + lx
                    if y < h and x < w and not np.isnan(rel[y, x]):
                        lanes[ly * 8 + lx] = rel[y, x]; cnt[ly * 8 + lx] = 1.0
            off = 32
            while off:
                lanes[:off] = lanes[:off] + lanes[off:2 * off]; cnt[:off] = cnt[:off] + cnt[off:2 * off]
                off //= 2
            out[ty, tx] = lanes[0] / cnt[0] if cnt[0] > 0 else 0.0
    return out


def pick_tau(means):
    """a tau between two neighbouring tile means near the median, far (relatively) from both"""
    m = np.sort(means.ravel())
    k = len(m) // 2
    for j in list(range(k, len(m) - 1)) + list(range(k - 1, 0, -1)):
        if m[j + 1] > m[j] * (1 + 1e-6) + 1e-300:
            return 0.5 * (m[j] + m[j + 1])
    raise AssertionError("no gap between the tile means")


def tile_mask(retired, w=W, h=H):
    return np.kron(retired, np.ones((8, 8), bool))[:h, :w]


def frozen_figures(cs, retire_at, iters, pm, active_var, composite, light, active_v=None):
    """numpy's restatement of tiles retired after `retire_at` of `iters` iterations (cs[j]: the plain run's sums after j iterations, one fold
    per iteration up to the retirement), at the 1 / iters scale, for any frame shape: the frozen variance of every pixel as if its tile had
    retired, and the three figures of the variance image that is frozen where pm (h, w) says so and active_var elsewhere.  active_v: the
    active pixels' v before the clamp -- with it a pixel is broken by the retired form's v where pm says so and by active_v elsewhere"""
    s = np.float64(np.float32(1.0 / iters))
    v_t, K_t = moments(cs[:retire_at + 1])
    f = (s * np.float64(iters)) / np.float64(retire_at)
    frozen = variance(v_t, (f * f) * K_t)
    v = None if active_v is None else np.where(pm[..., None], v_t, active_v)
    num, rel = rel_of(np.where(pm[..., None], frozen, active_var), composite, light, v=v)
    return frozen, (num.sum() / num.size, rel.sum() / num.size, rel.sum() / num.size)


def run(evplp, jp, sd, tau=None, vsl=False, runner=None, dealt=False):
    """ITERS iterations, a fold after each; with tau: adaptivity on, one retirement after iteration RETIRE_AT at the loop's 1 / i scale.
    Returns the accumulators after RETIRE_AT and ITERS iterations, the sums after every iteration, figures and statistics."""
    own = runner is None
    c = runner or evplp.Context(W, H, NL, NV, P, deterministic=True)
    group = not own
    try:
        c.load_scene_json(jp)
        if own:
            bsr, total, _ = c.scene_metrics()
        else:
            with evplp.Context(W, H, NL, NV, P) as m:
                m.load_scene_json(jp); bsr, total, _ = m.scene_metrics()
        fp_of = (lambda i: vsl_params(evplp, sd, bsr, total, i)) if vsl else (lambda i: params(evplp, sd, bsr, total, i))
        if dealt:
            c.calibrate(True); one_iteration(c, fp_of(0), 0, True, vsl); c.rebalance()
        c.clear_accumulators()
        c.noise_track(True)
        if tau is not None:
            c.adaptive_enable(True)
        out = dict(cs=[], retired=None)
        acc = (lambda: (c.resolve(1.0, 0.0, 0.0)[:H], c.resolve(0.0, 1.0, 0.0)[:H])) if group else \
              (lambda: (c.download(evplp.BUF_VPL_ACCUM)[:H], c.download(evplp.BUF_PHOTON_ACCUM)[:H]))
        if own:
            out["cs"].append(sums(evplp, c))
        for i in range(ITERS):
            one_iteration(c, fp_of(i), i, group, vsl)
            c.noise_fold(1)
            if own:
                out["cs"].append(sums(evplp, c))
            if i + 1 == RETIRE_AT:
                s = 1.0 / RETIRE_AT
                out["at"] = acc()
                out["composite_at"] = c.resolve(s, s, 1.0)[:H]
                out["est_at"] = c.noise_estimate(s)
                if tau is not None:
                    out["retired"] = c.adaptive_retire(s, tau, MIN_BATCHES)
                    out["tiles"] = c.adaptive_tiles()
            if i + 1 == ITERS - 4 and tau is not None:
                out["var_8"] = c.noise_variance(1.0 / (ITERS - 4))[:H]
        s = 1.0 / ITERS
        out["end"] = acc()
        out["stats"] = None if group else c.pass_stats(evplp.PASS_GATHER_VSL if vsl else evplp.PASS_GATHER_VPL)
        out["light"] = c.download(evplp.BUF_LIGHT)[:H] if own else None
        out["composite"] = c.resolve(s, s, 1.0)[:H]
        out["est"] = c.noise_estimate(s)
        out["var"] = c.noise_variance(s)[:H]
        if tau is not None:
            out["tiles_end"] = c.adaptive_tiles()
        return out
    finally:
        if own:
            c.close()


@pytest.fixture(scope="module")
def plain_and_adaptive(evplp, scene):
    jp, sd = scene
    plain = run(evplp, jp, sd)
    v, K = moments(plain["cs"][:RETIRE_AT + 1])
    s = np.float64(np.float32(1.0 / RETIRE_AT))
    _, rel = rel_of(variance(v, s * s * K), plain["composite_at"], plain["light"])
    means = tile_means(rel)
    tau = pick_tau(means)
    adaptive = run(evplp, jp, sd, tau=tau)
    return plain, adaptive, means, tau


def test_active_tiles_bit_identical_and_retired_pixels_extrapolated(plain_and_adaptive):
    plain, ad, means, tau = plain_and_adaptive
    retired = means <= tau
    assert 0 < retired.sum() < retired.size
    assert ad["retired"] == int(retired.sum())
    assert np.array_equal(ad["tiles"], np.where(retired, RETIRE_AT, RETIRE_AT))
    assert np.array_equal(ad["tiles_end"], np.where(retired, RETIRE_AT, ITERS))
    pm = tile_mask(retired)
    vpl_p, ph_p = plain["end"]; vpl_a, ph_a = ad["end"]
    assert vpl_a[~pm].tobytes() == vpl_p[~pm].tobytes()                   # active tiles: bit for bit
    assert ph_a.tobytes() == ph_p.tobytes()                               # the whole photon accumulator
    R = plain["at"][0].astype(np.float64)
    want = (R * (np.float64(ITERS) / np.float64(RETIRE_AT))).astype(np.float32)
    assert vpl_a[pm].tobytes() == want[pm].tobytes()                      # retired: the extrapolated snapshot
    # fewer shadow rays and shaded pairs in the last gather
    assert ad["stats"]["rays"] < plain["stats"]["rays"] and ad["stats"]["shaded"] < plain["stats"]["shaded"]


def test_frozen_noise_of_retired_pixels(plain_and_adaptive):
    plain, ad, means, tau = plain_and_adaptive
    retired = means <= tau
    pm = tile_mask(retired)
    s = np.float64(np.float32(1.0 / ITERS))
    v, K = moments(plain["cs"])
    # frozen figures for retired pixels, the tracker's for active ones
    frozen, want = frozen_figures(plain["cs"], RETIRE_AT, ITERS, pm, variance(v, s * s * K), ad["composite"], plain["light"])
    assert ad["var"][pm].tobytes() == frozen.astype(np.float32)[pm].tobytes()
    assert ad["var"][~pm].tobytes() == plain["var"][~pm].tobytes()        # active pixels as the plain run
    # the retired figure stays put as the run goes on (1 / N scale: the figure at retirement)
    np.testing.assert_allclose(ad["var_8"][pm], ad["var"][pm], rtol=1e-5, atol=0)
    # the estimate against numpy
    for g, w in zip(ad["est"], want):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1e-30), (ad["est"], want)


def test_all_tiles_retired_gather_nothing(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True)
        for i in range(3):
            one_iteration(c, params(evplp, sd, bsr, total, i), i, False); c.noise_fold(1)
        assert c.adaptive_retire(1.0 / 3, 1e300, 2) == TX * TY
        assert c.adaptive_retire(1.0 / 3, 1e300, 2) == 0                  # one-way: nothing left to retire
        before = c.download(evplp.BUF_VPL_ACCUM)[:H].astype(np.float64)
        one_iteration(c, params(evplp, sd, bsr, total, 3), 3, False)
        st = c.pass_stats(evplp.PASS_GATHER_VPL)
        assert st["rays"] == 0 and st["shaded"] == 0
        assert c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes() == (before * (4.0 / 3.0)).astype(np.float32).tobytes()
        assert np.array_equal(c.adaptive_tiles(), np.full((TY, TX), 3, np.int32))
        c.clear_accumulators()                                            # every tile active again, N = 0
        assert np.array_equal(c.adaptive_tiles(), np.zeros((TY, TX), np.int32))


@pytest.mark.parametrize("ranks, dealt", [(2, False), (3, True)])
def test_strips_decide_as_one_context(evplp, scene, plain_and_adaptive, ranks, dealt):
    jp, sd = scene
    _, ad, _, tau = plain_and_adaptive
    with evplp.Group(W, H, NL, NV, P, ranks, devices=[0] * ranks, deterministic=True) as g:
        gr = run(evplp, jp, sd, tau=tau, runner=g, dealt=dealt)
    assert gr["retired"] == ad["retired"]
    assert np.array_equal(gr["tiles_end"], ad["tiles_end"])
    assert gr["end"][0].tobytes() == ad["end"][0][..., :3].tobytes()
    assert gr["end"][1].tobytes() == ad["end"][1][..., :3].tobytes()
    assert gr["est"] == ad["est"] and gr["est_at"] == ad["est_at"]
    assert gr["var"].tobytes() == ad["var"].tobytes()


def test_vsl_active_tiles_bit_identical(evplp, scene):
    jp, sd = scene
    plain = run(evplp, jp, sd, vsl=True)
    v, K = moments(plain["cs"][:RETIRE_AT + 1])
    s = np.float64(np.float32(1.0 / RETIRE_AT))
    _, rel = rel_of(variance(v, s * s * K), plain["composite_at"], plain["light"])
    means = tile_means(rel)
    tau = pick_tau(means)
    ad = run(evplp, jp, sd, tau=tau, vsl=True)
    retired = means <= tau
    assert ad["retired"] == int(retired.sum()) and 0 < retired.sum() < retired.size
    pm = tile_mask(retired)
    assert ad["end"][0][~pm].tobytes() == plain["end"][0][~pm].tobytes()
    assert ad["end"][1].tobytes() == plain["end"][1].tobytes()
    R = plain["at"][0].astype(np.float64)
    assert ad["end"][0][pm].tobytes() == (R * (np.float64(ITERS) / np.float64(RETIRE_AT))).astype(np.float32)[pm].tobytes()
    assert ad["stats"]["rays"] < plain["stats"]["rays"]


def test_refusals_leave_the_context_usable(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        fp_of = lambda i: params(evplp, sd, bsr, total, i)
        c.clear_accumulators()
        with pytest.raises(evplp.EvplpError) as e:
            c.adaptive_enable(True)                                       # no noise tracking
        assert e.value.status == evplp.ERR_INVALID
        c.noise_track(True)
        one_iteration(c, fp_of(0), 0, False)
        with pytest.raises(evplp.EvplpError) as e:
            c.adaptive_enable(True)                                       # N = 1
        assert e.value.status == evplp.ERR_INVALID
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True)
        one_iteration(c, fp_of(0), 0, False)
        for call in (lambda: c.adaptive_enable(False), lambda: c.noise_track(True), lambda: c.noise_track(False),
                     lambda: c.gather_lvc(fp_of(1)), lambda: c.path_trace(sd.cam_origin, 1, 3)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID
        fp = fp_of(1); fp.do_accumulate = 0
        with pytest.raises(evplp.EvplpError) as e:
            c.gather_vpl(fp)
        assert e.value.status == evplp.ERR_INVALID
        one_iteration(c, fp_of(1), 1, False); c.noise_fold(1)             # still renders
        img = c.resolve(0.5, 0.5, 1.0)[:H]
        assert np.isfinite(img).all() and img.max() > 0
        assert np.array_equal(c.adaptive_tiles(), np.full((TY, TX), 2, np.int32))
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True, partition="iterations") as g:
        g.load_scene_json(jp)
        g.clear_accumulators(); g.noise_track(True)
        for call in (lambda: g.adaptive_enable(True), lambda: g.adaptive_retire(1.0, 0.1, 2), lambda: g.adaptive_tiles()):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID
        one_iteration(g, params(evplp, sd, bsr, total, 0), 0, True)       # the group stays usable
        assert np.isfinite(g.resolve(1.0, 1.0, 1.0)).all()


def _render(evplp, d, jp_src, block):
    write_inputs(evplp, d, jp_src)
    root = json.load(open(jp_src))
    root["photonfam"].update(numMaxIteration=12, numLightPaths=NL, numVplLightPaths=NV, radiusPercentage=0.05, misMode="balance",
                             DoProgressive=False, deterministic=True, combinedFilename="c.pfm", weightedPhotonFilename="pm.pfm",
                             weightedVplFilename="vpl.pfm", statFilename="s.json", run=dict(photonSplat=True))
    root["photonfam"].update(block)
    jp = d / "room.json"
    json.dump(root, open(jp, "w"))
    evplp.render_json(str(jp))
    return np.ascontiguousarray(evplp.load_pfm(str(d / "c.pfm")))


def test_technique_block(evplp, scene, tmp_path, plain_and_adaptive):
    jp, _ = scene
    tau = plain_and_adaptive[3]
    noise = {"batchIterations": 2, "everyIterations": 4, "filename": "noise.json"}
    plain = _render(evplp, tmp_path / "plain", jp, {"noise": noise})
    adaptive = _render(evplp, tmp_path / "adaptive", jp, {"noise": noise, "adaptive": {"tileRelMse": tau, "everyIterations": 4, "minBatches": 2,
                                                                                       "iterationsFilename": "iters.pfm"}})
    d = tmp_path / "adaptive"
    iters = evplp.load_pfm(str(d / "iters.pfm"))                          # (top-down, as c.pfm)
    cps = json.load(open(d / "noise.json"))["checkpoints"]
    assert all("retiredTiles" in p and p["retiredTiles"] + p["activeTiles"] == TX * TY for p in cps)
    assert "retiredTiles" not in json.load(open(tmp_path / "plain" / "noise.json"))["checkpoints"][0]
    # (a tile retired at the last iteration has n_t = N: 1 in the file, like a tile that never retired -- and its pixels still hold the sums
    # of every iteration, so both equal the plain run's)
    never = iters[..., 0] == 1.0
    retired_before = int((iters[::8, ::8, 0] < 1.0).sum())
    assert [p["iteration"] for p in cps] == [4, 8, 12]
    assert retired_before == cps[1]["retiredTiles"] <= cps[2]["retiredTiles"]
    assert adaptive[never].tobytes() == plain[never].tobytes()
    assert set(np.unique(iters[..., 0]).tolist()) <= {1.0} | {k / 12.0 for k in range(1, 12)} | {np.float32(k / 12.0).item() for k in range(1, 12)}
