"""EVPLP_PARTITION_ITERATIONS (include/evplp.h): the ranks of an evplp_group share out the iterations of a progressive run, and a
written frame is the sum of their accumulators -- formed on the GPUs in rank order (reduce_shards_kernel), the emitter plane as the
first non-zero pixel in rank order.  The sums are checked bit for bit against numpy, against one context (VPL / photon to fp32
round-off, the emitter image exactly) and against themselves (no second exchange without a pass, a time-limited run repeated by count).

The scene is the synthesized room with an extra occluder just below part of the ceiling light: the light plane of an accumulating run
is the union over the iterations of the pixels where the un-jittered emitter passes the depth test against the jittered scene, so at
the occluder's edge one rank's iterations do not light every pixel all iterations light."""
import json
import math
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H, P, NL, NV, ITERS = 96, 64, 4, 2048, 40, 7


def occluded_room(evplp, d):
    """The synthesized room (96 x 64) and a quad 5 cm below the ceiling light that hides its half at x < 5."""
    jp = evplp.synth_scene(str(d), "room", 3000, 3, W, H, style="hard")
    obj = os.path.join(str(d), "room.obj")
    lines = open(obj).read().splitlines()
    nv = sum(1 for l in lines if l.startswith("v ")); nt = sum(1 for l in lines if l.startswith("vt "))
    quad = [(-1.7, -2.1), (5.0, -2.1), (5.0, 4.1), (-1.7, 4.1)]
    add = ["usemtl obj0"] + [f"v {x} {y} 6.40\nvt 0 0" for x, y in quad]
    add += [f"f {nv + 1}/{nt + 1} {nv + 2}/{nt + 2} {nv + 3}/{nt + 3}", f"f {nv + 1}/{nt + 1} {nv + 3}/{nt + 3} {nv + 4}/{nt + 4}"]
    open(obj, "w").write("\n".join(lines + add) + "\n")
    return jp


def frame_params(evplp, sd, bsr, total, it, jitter):
    r = 0.05 * bsr
    return evplp.frame_params(camera_pos=sd.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), clamping_value=1.0 / total,
                              photon_radius=r, num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=it,
                              jitter=tuple(float(x) for x in jitter))


def run_group(evplp, jp, sd, n, devices=None, iters=ITERS, **kw):
    """n iteration ranks, iteration i on rank i % n; returns the open group (the caller closes it)"""
    g = evplp.Group(W, H, NL, NV, P, n, devices=devices if devices is not None else [0] * n, deterministic=True, partition="iterations", **kw)
    g.load_scene_json(jp)
    bsr, total, _ = g.context(0).scene_metrics()
    js = evplp.jitter_sequence(0, iters, W, H)
    g.clear_accumulators()
    for i in range(iters):
        g.select_rank(i % n)
        fp = frame_params(evplp, sd, bsr, total, i, js[i])
        g.primary(tuple(js[i])); g.trace_light_paths(i); g.gather(fp, 0); g.splat_photons(fp)
    return g


def rank_planes(evplp, g):
    return [{b: g.context(r).download(b)[:H] for b in (evplp.BUF_VPL_ACCUM, evplp.BUF_PHOTON_ACCUM, evplp.BUF_LIGHT)} for r in range(g.n)]


def expected_sums(evplp, planes):
    vpl, pm, light = (planes[0][b].copy() for b in (evplp.BUF_VPL_ACCUM, evplp.BUF_PHOTON_ACCUM, evplp.BUF_LIGHT))
    for p in planes[1:]:
        vpl = vpl + p[evplp.BUF_VPL_ACCUM]          # float32 adds in rank order
        pm = pm + p[evplp.BUF_PHOTON_ACCUM]
        take = ~(light != 0).any(-1) & (p[evplp.BUF_LIGHT] != 0).any(-1)
        light[take] = p[evplp.BUF_LIGHT][take]
    return vpl, pm, light


def test_rank_order_reduction_bit_for_bit(evplp, tmp_path):
    jp = occluded_room(evplp, tmp_path)
    sd, _ = scenes.load_obj_scene(jp)
    with run_group(evplp, jp, sd, 3, overlap_light_tracing=True) as g:
        planes = rank_planes(evplp, g)
        vpl, pm, light = expected_sums(evplp, planes)
        assert vpl.max() > 0 and pm.max() > 0 and light.max() > 0
        assert all(p[evplp.BUF_VPL_ACCUM].max() > 0 for p in planes)
        assert np.array_equal(g.resolve(1.0, 0.0, 0.0), vpl[..., :3])
        assert np.array_equal(g.resolve(0.0, 1.0, 0.0), pm[..., :3])
        assert np.array_equal(g.resolve(0.0, 0.0, 1.0), light[..., :3])
        s = 1.0 / ITERS
        img = g.resolve(s, s, 1.0)
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        pad = np.zeros((c.local_rows, W, 4), np.float32)
        for b, plane in ((evplp.BUF_VPL_ACCUM, vpl), (evplp.BUF_PHOTON_ACCUM, pm), (evplp.BUF_LIGHT, light)):
            full = pad.copy(); full[:H] = plane
            c.upload(b, full)
        ref = c.resolve(s, s, 1.0)[:H]
    assert img.tobytes() == ref.tobytes()


def test_equal_to_one_context_and_the_emitter_image_exactly(evplp, tmp_path):
    jp = occluded_room(evplp, tmp_path)
    sd, _ = scenes.load_obj_scene(jp)
    with run_group(evplp, jp, sd, 3) as g:
        planes = rank_planes(evplp, g)
        vpl, pm, light = expected_sums(evplp, planes)
        img = g.resolve(0.0, 0.0, 1.0)
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        js = evplp.jitter_sequence(0, ITERS, W, H)
        c.clear_accumulators()
        for i in range(ITERS):
            fp = frame_params(evplp, sd, bsr, total, i, js[i])
            c.primary(tuple(js[i])); c.trace_light_paths(i); c.gather_vpl(fp); c.splat_photons(fp)
        one = {b: c.download(b)[:H] for b in (evplp.BUF_VPL_ACCUM, evplp.BUF_PHOTON_ACCUM, evplp.BUF_LIGHT)}
    # the precondition: rank 0 alone (iterations 0, 3, 6) misses emitter pixels that the seven iterations light
    assert not np.array_equal(planes[0][evplp.BUF_LIGHT], one[evplp.BUF_LIGHT]), "the occluder does not make the ranks' emitter planes differ"
    assert np.array_equal(light, one[evplp.BUF_LIGHT])
    assert np.array_equal(img, one[evplp.BUF_LIGHT][..., :3])
    for got, b in ((vpl, evplp.BUF_VPL_ACCUM), (pm, evplp.BUF_PHOTON_ACCUM)):
        ref = one[b].astype(np.float64)
        assert ref.max() > 0
        assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-6, b


def test_no_second_exchange_without_a_pass(evplp, tmp_path):
    jp = occluded_room(evplp, tmp_path)
    sd, _ = scenes.load_obj_scene(jp)
    with run_group(evplp, jp, sd, 3, iters=3) as g:
        a = g.resolve(0.5, 0.5, 1.0)
        before = [g.host_stats(r)["exchange_ms"] for r in range(3)]
        b = g.resolve(0.25, 0.0, 1.0)
        g.present(1.0, 1.0, 1.0)
        assert [g.host_stats(r)["exchange_ms"] for r in range(3)] == before
        assert not np.array_equal(a, b)
        g.select_rank(1)
        g.primary((0.001, 0.001))
        c = g.resolve(0.5, 0.5, 1.0)
        after = [g.host_stats(r)["exchange_ms"] for r in range(3)]
        assert all(x > y for x, y in zip(after, before)), (before, after)
        assert np.isfinite(c).all()


def test_refusals_leave_the_group_usable(evplp, tmp_path):
    jp = occluded_room(evplp, tmp_path)
    sd, _ = scenes.load_obj_scene(jp)
    with evplp.Group(W, H, NL, NV, P, 2, devices=[0, 0], deterministic=True) as g:        # strips
        g.load_scene_json(jp)
        with pytest.raises(evplp.EvplpError):
            g.select_rank(0)
        bsr, total, _ = g.context(0).scene_metrics()
        fp = frame_params(evplp, sd, bsr, total, 0, (0.0, 0.0))
        g.primary(); g.trace_light_paths(0); g.gather(fp, 0)
        assert g.resolve(1.0, 0.0, 1.0).max() > 0
    with pytest.raises(evplp.EvplpError):
        evplp.Group(W, H, NL, NV, P, 2, devices=[0, 0], partition="iterations", split_light_paths=1)
    with run_group(evplp, jp, sd, 3, iters=2) as g:
        for refused in (lambda: g.calibrate(True), g.rebalance, g.block_owners, lambda: g.select_rank(3), lambda: g.select_rank(-1),
                        lambda: g.synchronize_rank(3)):
            with pytest.raises(evplp.EvplpError):
                refused()
        g.synchronize_rank(1)
        g.select_rank(2)
        bsr, total, _ = g.context(0).scene_metrics()
        fp = frame_params(evplp, sd, bsr, total, 2, (0.0, 0.0))
        g.primary(); g.trace_light_paths(2); g.gather(fp, 0); g.splat_photons(fp)
        img = g.resolve(1.0 / 3, 1.0 / 3, 1.0)
        assert np.isfinite(img).all() and img.max() > 0
    with evplp.Group(W, H, NL, NV, P, 1, devices=[0], partition="iterations") as g:
        g.rebalance()                                                                       # (a single rank: nothing to deal, no error)


def render(evplp, d, jp_src, device, **block):
    d.mkdir()
    root = json.load(open(jp_src))
    for f in ("room.obj", "room.mtl", "room_lights.obj"):
        (d / f).write_bytes(open(os.path.join(os.path.dirname(jp_src), f), "rb").read())
    root["photonfam"].update(numMaxIteration=ITERS, numLightPaths=NL, numVplLightPaths=NV, radiusPercentage=0.05, misMode="balance", DoProgressive=True,
                             deterministic=True, device=device, combinedFilename="c.pfm", weightedPhotonFilename="pm.pfm", weightedVplFilename="vpl.pfm",
                             statFilename="s.json", run=dict(photonSplat=True))
    root["photonfam"].update(block)
    jp = d / "room.json"
    json.dump(root, open(jp, "w"))
    evplp.render_json(str(jp))
    return {f: evplp.load_pfm(str(d / f)) for f in ("c.pfm", "pm.pfm", "vpl.pfm")}, json.load(open(d / "s.json"))


def test_render_json_matches_the_one_gpu_emitter(evplp, tmp_path):
    (tmp_path / "src").mkdir()
    jp = occluded_room(evplp, tmp_path / "src")
    one, _ = render(evplp, tmp_path / "one", jp, dict(gpus=1))
    three, st = render(evplp, tmp_path / "three", jp, dict(gpus=3, virtual=True, partition="iterations"))
    assert st["numIterations"] == ITERS
    light = np.asarray(json.load(open(jp))["arealight"]["intensity"][:3], np.float32)
    emitter = (one["vpl.pfm"] >= 0.5 * light).all(-1)          # (the emitter's pixels carry its colour: the light surface reflects nothing)
    assert emitter.sum() > 10
    for f in ("c.pfm", "vpl.pfm"):
        assert np.array_equal(three[f][emitter], one[f][emitter]), f
    for f, ref in one.items():
        assert ref.max() > 0, f
        rel = np.linalg.norm(three[f].astype(np.float64) - ref) / np.linalg.norm(ref)
        assert rel < 1e-6, (f, rel)


def test_time_limited_run_loses_and_repeats_no_iteration(evplp, tmp_path):
    (tmp_path / "src").mkdir()
    jp = occluded_room(evplp, tmp_path / "src")
    dev = dict(gpus=3, virtual=True, partition="iterations")
    timed, st = render(evplp, tmp_path / "timed", jp, dev, timeLimitMs=1500, numMaxIteration=-1)
    n = int(st["numIterations"])
    assert n >= 3
    counted, st2 = render(evplp, tmp_path / "counted", jp, dev, numMaxIteration=n)
    assert int(st2["numIterations"]) == n
    for f in timed:
        assert timed[f].tobytes() == counted[f].tobytes(), f


def test_distinct_devices_equal_virtual_ranks(evplp, tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    jp = occluded_room(evplp, tmp_path)
    sd, _ = scenes.load_obj_scene(jp)
    imgs = []
    for devices in ([0, 1], [0, 0]):
        with run_group(evplp, jp, sd, 2, devices=devices) as g:
            imgs.append(g.resolve(0.5, 0.5, 1.0))
    assert imgs[0].max() > 0 and imgs[0].tobytes() == imgs[1].tobytes()
