"""Adaptive sampling for the path tracer (evplp_adaptive_enable_pt, evplp_group_adaptive_enable_pt and the pt technique's "adaptiveSampling"
block) on the 96 x 64 room of tests/test_gpu_convergence.py.

A plain run and an adaptive run of the same path-traced iterations are compared, everything exactly: active tiles bit for bit, retired pixels
against numpy's extrapolation of the plain run's accumulator, the set of retired tiles against numpy's restatement of the criterion, the pass
counters against a count formed from the G-buffer, the frozen variance of retired pixels bit for bit; nothing traced when every tile has
retired; row strips of 2 and 3 virtual ranks against one context (the denoiser too); every refusal; and the technique loop's block."""
import json

import numpy as np
import pytest

from test_gpu_adaptive import (ITERS, MIN_BATCHES, RETIRE_AT, TX, TY, moments, one_iteration, pick_tau, rel_of, scene, sums,  # noqa: F401
                               tile_mask, tile_means, variance)
from test_gpu_convergence import NL, NV, P, H, W, params, write_inputs

pytestmark = pytest.mark.gpu

JITTER = (0.002, -0.001)
GBUF = ("BUF_GBUF_POSITION", "BUF_GBUF_NORMAL", "BUF_GBUF_DIFFUSE", "BUF_GBUF_PHONG")


def iteration(runner, cam, i):
    runner.primary(JITTER); runner.path_trace(cam, i, 3); runner.noise_fold(1)


def run(evplp, jp, sd, tau=None, runner=None, dealt=False):
    """ITERS path-traced iterations, a fold after each; with tau: path-trace mode, one retirement after iteration RETIRE_AT at scale
    1 / RETIRE_AT.  Returns the accumulators after RETIRE_AT and ITERS iterations, the sums after every iteration, figures and statistics."""
    own = runner is None
    c = runner or evplp.Context(W, H, NL, NV, P, deterministic=True)
    try:
        c.load_scene_json(jp)
        if dealt:
            with evplp.Context(W, H, NL, NV, P) as m:
                m.load_scene_json(jp); bsr, total, _ = m.scene_metrics()
            c.calibrate(True); one_iteration(c, params(evplp, sd, bsr, total, 0), 0, True); c.rebalance()
        c.clear_accumulators()
        c.noise_track(True)
        if tau is not None:
            c.adaptive_enable(True, path_trace=True)
        out = dict(cs=[], retired=None)
        acc = (lambda: (c.download(evplp.BUF_VPL_ACCUM)[:H], c.download(evplp.BUF_PHOTON_ACCUM)[:H])) if own else \
              (lambda: (c.resolve(1.0, 0.0, 0.0)[:H], c.resolve(0.0, 1.0, 0.0)[:H]))
        if own:
            out["cs"].append(sums(evplp, c))
        for i in range(ITERS):
            iteration(c, sd.cam_origin, i)
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
        s = 1.0 / ITERS
        out["end"] = acc()
        out["composite"] = c.resolve(s, s, 1.0)[:H]
        out["est"] = c.noise_estimate(s)
        out["var"] = c.noise_variance(s)[:H]
        out["den"] = c.denoise(s)[:H]
        if own:
            out["stats"] = c.pass_stats(evplp.PASS_PATH_TRACE)
            out["light"] = c.download(evplp.BUF_LIGHT)[:H]
            out["gbuf"] = [c.download(getattr(evplp, b))[:H] for b in GBUF]
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
    print(f"tile means {means.min():.4g} .. {means.max():.4g}, tau {tau:.6g}, retired {int(retired.sum())} of {retired.size}")
    assert 0 < retired.sum() < retired.size
    assert ad["retired"] == int(retired.sum())
    assert np.array_equal(ad["tiles"], np.full((TY, TX), RETIRE_AT, np.int32))
    assert np.array_equal(ad["tiles_end"], np.where(retired, RETIRE_AT, ITERS))
    pm = tile_mask(retired)
    vpl_p, ph_p = plain["end"]; vpl_a, ph_a = ad["end"]
    assert vpl_a[~pm].tobytes() == vpl_p[~pm].tobytes()                   # active tiles: bit for bit
    R = plain["at"][0].astype(np.float64)
    want = (R * (np.float64(ITERS) / np.float64(RETIRE_AT))).astype(np.float32)
    assert vpl_a[pm].tobytes() == want[pm].tobytes()                      # retired: the extrapolated snapshot
    assert ph_a.tobytes() == ph_p.tobytes() and not ph_a.any()            # the photon plane: untouched
    assert ad["light"].tobytes() == plain["light"].tobytes()
    for a, b in zip(ad["gbuf"], plain["gbuf"]):
        assert a.tobytes() == b.tobytes()


def test_pass_counters_count_the_active_tiles_only(evplp, plain_and_adaptive):
    plain, ad, means, tau = plain_and_adaptive
    pm = tile_mask(means <= tau)
    surface = plain["gbuf"][0][..., 3] != 0.0
    assert plain["stats"]["pairs"] == int(surface.sum())
    assert ad["stats"]["pairs"] == int((surface & ~pm).sum())
    assert 0 < ad["stats"]["rays"] < plain["stats"]["rays"]


def test_all_tiles_retired_trace_nothing(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, path_trace=True)
        for i in range(3):
            iteration(c, sd.cam_origin, i)
        assert c.adaptive_retire(1.0 / 3, 1e300, 2) == TX * TY
        assert c.adaptive_retire(1.0 / 3, 1e300, 2) == 0                  # one-way: nothing left to retire
        before = c.download(evplp.BUF_VPL_ACCUM)[:H].astype(np.float64)
        c.primary(JITTER); c.path_trace(sd.cam_origin, 3, 3)
        st = c.pass_stats(evplp.PASS_PATH_TRACE)
        assert st["rays"] == 0 and st["pairs"] == 0
        assert c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes() == (before * (4.0 / 3.0)).astype(np.float32).tobytes()
        assert np.array_equal(c.adaptive_tiles(), np.full((TY, TX), 3, np.int32))
        c.clear_accumulators()                                            # every tile active again, N = 0
        assert np.array_equal(c.adaptive_tiles(), np.zeros((TY, TX), np.int32))
        c.primary(JITTER); c.path_trace(sd.cam_origin, 0, 3)
        assert c.pass_stats(evplp.PASS_PATH_TRACE)["rays"] > 0


def test_frozen_noise_of_retired_pixels(plain_and_adaptive):
    plain, ad, means, tau = plain_and_adaptive
    pm = tile_mask(means <= tau)
    s = np.float64(np.float32(1.0 / ITERS))
    v_t, K_t = moments(plain["cs"][:RETIRE_AT + 1])
    f = (s * np.float64(ITERS)) / np.float64(RETIRE_AT)
    frozen = variance(v_t, (f * f) * K_t)
    assert ad["var"][pm].tobytes() == frozen.astype(np.float32)[pm].tobytes()
    assert ad["var"][~pm].tobytes() == plain["var"][~pm].tobytes()        # active pixels as the plain run
    # the estimate against numpy: frozen figures for retired pixels, the tracker's for active ones
    v, K = moments(plain["cs"])
    var = np.where(pm[..., None], frozen, variance(v, s * s * K))
    num, rel = rel_of(var, ad["composite"], plain["light"])
    want = (num.sum() / num.size, rel.sum() / num.size, rel.sum() / num.size)
    for g, w in zip(ad["est"], want):
        assert abs(g - w) <= 1e-12 * max(abs(w), 1e-30), (ad["est"], want)


@pytest.mark.parametrize("ranks, dealt", [(2, False), (3, True)])
def test_strips_decide_as_one_context(evplp, scene, plain_and_adaptive, ranks, dealt):
    jp, sd = scene
    _, ad, _, tau = plain_and_adaptive
    with evplp.Group(W, H, NL, NV, P, ranks, devices=[0] * ranks, deterministic=True) as g:
        gr = run(evplp, jp, sd, tau=tau, runner=g, dealt=dealt)
    assert gr["retired"] == ad["retired"]
    assert np.array_equal(gr["tiles"], ad["tiles"]) and np.array_equal(gr["tiles_end"], ad["tiles_end"])
    assert gr["end"][0].tobytes() == ad["end"][0][..., :3].tobytes()
    assert gr["end"][1].tobytes() == ad["end"][1][..., :3].tobytes()
    assert gr["est"] == ad["est"] and gr["est_at"] == ad["est_at"]
    assert gr["var"].tobytes() == ad["var"].tobytes()
    assert gr["den"].tobytes() == ad["den"].tobytes()                     # Group.denoise in path-trace mode: Context.denoise


def _refused(evplp, calls):
    for call in calls:
        with pytest.raises(evplp.EvplpError) as e:
            call()
        assert e.value.status == evplp.ERR_INVALID, e.value


def test_refusals_leave_the_context_usable(evplp, scene):
    jp, sd = scene
    cam = sd.cam_origin
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        fp_of = lambda i: params(evplp, sd, bsr, total, i)
        c.clear_accumulators()
        _refused(evplp, [lambda: c.adaptive_enable(True, path_trace=True)])          # no noise tracking
        c.noise_track(True)
        c.primary(JITTER); c.path_trace(cam, 0, 3)
        # N = 1 after a path-tracing sample: neither mode can be switched on
        _refused(evplp, [lambda: c.adaptive_enable(True, path_trace=True), lambda: c.adaptive_enable(True)])
        c.clear_accumulators(); c.noise_track(True); c.adaptive_enable(True, path_trace=True)
        iteration(c, cam, 0)
        c.trace_light_paths(1)
        nacc = fp_of(1); nacc.do_accumulate = 0
        _refused(evplp, [lambda: c.gather_vpl(fp_of(1)), lambda: c.gather_vsl(fp_of(1)), lambda: c.gather_lvc(fp_of(1)), lambda: c.gather_vpl(nacc),
                         lambda: c.path_trace(cam, 1, 3, accumulate=False),
                         lambda: c.adaptive_enable(True), lambda: c.adaptive_enable(False), lambda: c.adaptive_enable(False, path_trace=True),
                         lambda: c.noise_track(True), lambda: c.noise_track(False)])
        iteration(c, cam, 1)                                              # still renders
        img = c.resolve(0.5, 0.5, 1.0)[:H]
        assert np.isfinite(img).all() and img.max() > 0
        assert np.array_equal(c.adaptive_tiles(), np.full((TY, TX), 2, np.int32))
        # a switch at N = 0 goes through, in both directions
        c.clear_accumulators(); c.adaptive_enable(True); c.adaptive_enable(True, path_trace=True); c.adaptive_enable(False, path_trace=True)
        c.primary(JITTER); c.path_trace(cam, 0, 3, accumulate=False)      # adaptivity off: as ever
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True) as g:
        g.load_scene_json(jp)
        g.clear_accumulators()
        _refused(evplp, [lambda: g.adaptive_enable(True, path_trace=True)])          # no noise tracking
        g.noise_track(True); g.adaptive_enable(True, path_trace=True)
        iteration(g, cam, 0)
        g.trace_light_paths(1)
        _refused(evplp, [lambda: g.gather(fp_of(1), 0), lambda: g.gather(fp_of(1), 1), lambda: g.gather(fp_of(1), 2),
                         lambda: g.path_trace(cam, 1, 3, accumulate=False), lambda: g.adaptive_enable(True), lambda: g.adaptive_enable(False, path_trace=True),
                         lambda: g.noise_track(True)])
        iteration(g, cam, 1)
        assert np.isfinite(g.resolve(0.5, 0.5, 1.0)).all()
        assert np.array_equal(g.adaptive_tiles(), np.full((TY, TX), 2, np.int32))
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0] * 2, deterministic=True, partition="iterations") as g:
        g.load_scene_json(jp)
        g.clear_accumulators(); g.noise_track(True)
        _refused(evplp, [lambda: g.adaptive_enable(True, path_trace=True), lambda: g.adaptive_enable(False, path_trace=True),
                         lambda: g.adaptive_retire(1.0, 0.1, 2), lambda: g.adaptive_tiles()])
        one_iteration(g, fp_of(0), 0, True)                               # the group stays usable
        assert np.isfinite(g.resolve(1.0, 1.0, 1.0)).all()


NOISE = {"batchIterations": 2, "everyIterations": 4, "filename": "noise.json"}


def _render(evplp, d, jp_src, **block):
    write_inputs(evplp, d, jp_src)
    root = json.load(open(jp_src))
    root.pop("photonfam")
    root["pt"] = dict(rngOffset=0, numMaxIteration=12, timeLimitMs=1e9, frameMode="accumulate", outputFilename="c.pfm", statFilename="s.json",
                      useJitter=True, useStat=True, numSamplePerPixel=1, numMaxBounces=3)
    root["pt"].update(block)
    jp = d / "room.json"
    json.dump(root, open(jp, "w"))
    evplp.render_json(str(jp))
    return np.ascontiguousarray(evplp.load_pfm(str(d / "c.pfm"))), json.load(open(d / "s.json")), json.load(open(d / "noise.json"))["checkpoints"]


def test_technique_block(evplp, scene, tmp_path, plain_and_adaptive):
    jp, _ = scene
    tau = plain_and_adaptive[3]
    plain, st_plain, cps_plain = _render(evplp, tmp_path / "plain", jp, noise=NOISE)
    block = {"tileRelMse": tau, "everyIterations": 4, "minBatches": 2, "iterationsFilename": "iters.pfm"}
    adaptive, st, cps = _render(evplp, tmp_path / "adaptive", jp, noise=NOISE, adaptiveSampling=block)
    d = tmp_path / "adaptive"
    iters = evplp.load_pfm(str(d / "iters.pfm"))                          # (top-down, as c.pfm)
    assert all(p["retiredTiles"] + p["activeTiles"] == TX * TY for p in cps)
    assert "retiredTiles" not in cps_plain[0]
    print("retired tiles at the checkpoints:", [(p["iteration"], p["retiredTiles"]) for p in cps])
    # the run goes its whole length (tiles stay active: tau sits at the median of the tile means after four samples) and some tile retires
    assert st["numIterations"] == st_plain["numIterations"] == 12 and sorted(st) == sorted(st_plain)
    assert [p["iteration"] for p in cps] == [p["iteration"] for p in cps_plain] == [4, 8, 12]
    assert 0 < cps[1]["retiredTiles"] < TX * TY
    # iters.pfm: n_t / N per tile, one value per tile and channel, 1 where the tile never retired (or retired at the last iteration)
    t = iters[::8, ::8, 0]
    assert np.array_equal(iters, np.repeat(np.kron(t, np.ones((8, 8), np.float32))[:H, :W, None], 3, axis=2))
    assert set(np.unique(t).tolist()) <= {np.float32(4.0 / 12.0).item(), np.float32(8.0 / 12.0).item(), 1.0}
    assert int((t == np.float32(4.0 / 12.0)).sum()) == cps[0]["retiredTiles"]
    assert int((t < 1.0).sum()) == cps[1]["retiredTiles"] <= cps[2]["retiredTiles"]
    never = iters[..., 0] == 1.0
    assert adaptive[never].tobytes() == plain[never].tobytes()            # active tiles: the plain run's image, bit for bit
    assert not np.array_equal(adaptive[~never], plain[~never])
    # every tile retired at once: the loop ends at the first due retirement with minBatches folds behind it (iteration 8: four folds of two)
    all_block = {"tileRelMse": 1e300, "everyIterations": 4, "minBatches": 3, "iterationsFilename": "iters.pfm"}
    ended, st_e, cps_e = _render(evplp, tmp_path / "ended", jp, noise=NOISE, adaptiveSampling=all_block)
    assert st_e["numIterations"] == 8 < 12
    assert [(p["iteration"], p["retiredTiles"]) for p in cps_e] == [(4, 0), (8, TX * TY)]
    eight, st_8, _ = _render(evplp, tmp_path / "eight", jp, noise=NOISE, numMaxIteration=8)
    assert st_8["numIterations"] == 8 and ended.tobytes() == eight.tobytes()
    assert np.array_equal(evplp.load_pfm(str(tmp_path / "ended" / "iters.pfm")), np.ones((H, W, 3), np.float32))
