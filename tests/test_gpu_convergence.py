"""Error against a reference image on the device (evplp_frame_error, evplp_group_frame_error and the technique JSON's "convergence" block).

The figures are checked against numpy over the frame resolve() returns -- the fp32 terms of floatimage.cpp:64-112 reproduced exactly, summed
in fp64 -- against themselves (one context, row strips round robin and dealt by cost: the same doubles bit for bit), and in the technique
loops: checkpoints where they are due, the written images untouched, stopRelMse and a time limit."""
import json
import math
import os

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H, P, NL, NV = 96, 64, 4, 2048, 40


def room(evplp, d, name="room"):
    return evplp.synth_scene(str(d), name, 3000, 3, W, H, style="hard")


def params(evplp, sd, bsr, total, it, jitter=(0.002, -0.001)):
    r = 0.05 * bsr
    return evplp.frame_params(camera_pos=sd.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), clamping_value=1.0 / total,
                              photon_radius=r, num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=it,
                              jitter=jitter)


def accumulate(runner, fp_of, iters, group):
    runner.clear_accumulators()
    for i in range(iters):
        fp = fp_of(i)
        runner.primary((0.002, -0.001)); runner.trace_light_paths(i)
        if group:
            runner.gather(fp, 0)
        else:
            runner.gather_vpl(fp)
        runner.splat_photons(fp)


def numpy_error(img, ref_top_down, mask_top_down=None):
    """img: (H, W, 3) y = 0 at the bottom, as resolve() returns it; the reference and the mask top-down"""
    img = img.astype(np.float32)
    ref = np.ascontiguousarray(ref_top_down[::-1]).astype(np.float32)
    d = img - ref
    num = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    den = ref[..., 0] * ref[..., 0] + ref[..., 1] * ref[..., 1] + ref[..., 2] * ref[..., 2] + np.float32(0.001)
    rel = num / den
    assert num.dtype == np.float32 and rel.dtype == np.float32
    keep = np.ones(num.shape, bool) if mask_top_down is None else mask_top_down[::-1].any(-1)
    n = num.size
    kept = int(keep.sum())
    return (num.astype(np.float64).sum() / n, rel.astype(np.float64).sum() / n,
            rel[keep].astype(np.float64).sum() / kept if kept else 0.0)


def close(got, want, tol):
    for g, w in zip(got, want):
        assert abs(g - w) <= tol * abs(w) + 1e-300, (got, want)


def reference_and_mask():
    mask = np.full((H, W, 3), 255, np.uint8)
    mask[10:22, :, :] = 0                       # a band of rows
    mask[30:40, 5:9, 1] = 7                     # kept: one non-zero byte is enough
    mask[30:40, 5:9, 0] = 0; mask[30:40, 5:9, 2] = 0
    return mask


@pytest.fixture(scope="module")
def scene(evplp, tmp_path_factory):
    d = tmp_path_factory.mktemp("conv_scene")
    jp = room(evplp, d)
    sd, _ = scenes.load_obj_scene(jp)
    return jp, sd


def test_context_against_numpy_itself_and_without_side_effects(evplp, scene):
    jp, sd = scene
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        with pytest.raises(evplp.EvplpError) as e:
            c.frame_error(1.0, 1.0, 1.0)
        assert "reference" in str(e.value)
        long_run = 6
        accumulate(c, lambda i: params(evplp, sd, bsr, total, 100 + i), long_run, False)
        ref = np.ascontiguousarray(c.resolve(1.0 / long_run, 1.0 / long_run, 1.0)[:H][::-1])
        ref[3, 4] = 0.0; ref[40, 50] = 0.0; ref[63, 95] = 0.0             # a few pixels where |ref|^2 is 0: the 0.001 alone is the denominator
        mask = reference_and_mask()
        n = 3
        accumulate(c, lambda i: params(evplp, sd, bsr, total, i), n, False)
        for with_mask in (False, True):
            c.set_error_reference(ref, mask if with_mask else None)
            for scales in ((1.0 / n, 1.0 / n, 1.0), (0.0, 1.0 / n, 0.0)):
                for gamma in (False, True):
                    for mask_emitter in (False, True):
                        img = c.resolve(*scales, mask_emitter=mask_emitter, gamma=gamma)[:H]
                        got = c.frame_error(*scales, mask_emitter=mask_emitter, gamma=gamma)
                        want = numpy_error(img, ref, mask if with_mask else None)
                        assert want[1] > 0
                        close(got, want, 1e-12)
                        if not with_mask:
                            assert got[2] == got[1]
        # the frame against itself: exactly zero
        s = 1.0 / n
        img = c.resolve(s, s, 1.0)[:H]
        c.set_error_reference(np.ascontiguousarray(img[::-1]), mask)
        assert c.frame_error(s, s, 1.0) == (0.0, 0.0, 0.0)
        # no side effects: the resolved frame and the three planes are the same bits before and after
        c.set_error_reference(ref, mask)
        planes = (evplp.BUF_VPL_ACCUM, evplp.BUF_PHOTON_ACCUM, evplp.BUF_LIGHT)
        before = [c.resolve(s, s, 1.0).tobytes()] + [c.download(b).tobytes() for b in planes]
        c.frame_error(s, 0.0, 1.0, mask_emitter=True, gamma=True)
        after = [c.resolve(s, s, 1.0).tobytes()] + [c.download(b).tobytes() for b in planes]
        assert before == after
        # a mask that keeps nothing: the masked figure is 0; releasing the reference makes the call an error again
        c.set_error_reference(ref, np.zeros((H, W, 3), np.uint8))
        assert c.frame_error(s, s, 1.0)[2] == 0.0
        c.set_error_reference(None)
        with pytest.raises(evplp.EvplpError):
            c.frame_error(s, s, 1.0)


def test_partition_independence_bit_for_bit(evplp, scene):
    jp, sd = scene
    n = 3
    mask = reference_and_mask()
    with evplp.Context(W, H, NL, NV, P, deterministic=True) as c:
        c.load_scene_json(jp)
        bsr, total, _ = c.scene_metrics()
        fp_of = lambda i: params(evplp, sd, bsr, total, i)
        accumulate(c, lambda i: params(evplp, sd, bsr, total, 50 + i), 5, False)
        ref = np.ascontiguousarray(c.resolve(0.2, 0.2, 1.0)[:H][::-1])
        accumulate(c, fp_of, n, False)
        c.set_error_reference(ref, mask)
        one = c.frame_error(1.0 / n, 1.0 / n, 1.0)
        one_plain = c.frame_error(0.0, 1.0 / n, 0.0, gamma=True)
        img = c.resolve(1.0 / n, 1.0 / n, 1.0)[:H]
    close(one, numpy_error(img, ref, mask), 1e-12)
    with evplp.Group(W, H, NL, NV, P, 4, devices=[0] * 4, deterministic=True) as g:
        g.load_scene_json(jp)
        with pytest.raises(evplp.EvplpError) as e:
            g.frame_error(1.0, 1.0, 1.0)                      # no reference: refused on the caller's thread ...
        assert "reference" in str(e.value)
        g.set_error_reference(ref, mask)
        accumulate(g, fp_of, n, True)                          # ... and the group is still usable
        assert g.frame_error(1.0 / n, 1.0 / n, 1.0) == one
        assert g.frame_error(0.0, 1.0 / n, 0.0, gamma=True) == one_plain
        g.calibrate(True)
        accumulate(g, fp_of, 1, True)
        g.rebalance()
        accumulate(g, fp_of, n, True)
        assert g.frame_error(1.0 / n, 1.0 / n, 1.0) == one
        assert g.frame_error(0.0, 1.0 / n, 0.0, gamma=True) == one_plain
        assert g.resolve(1.0 / n, 1.0 / n, 1.0).tobytes() == img.tobytes()
    # the iteration partition: numpy over its own resolve()
    with evplp.Group(W, H, NL, NV, P, 3, devices=[0] * 3, deterministic=True, partition="iterations") as g:
        g.load_scene_json(jp)
        g.set_error_reference(ref, mask)
        g.clear_accumulators()
        for i in range(5):
            g.select_rank(i % 3)
            fp = fp_of(i)
            g.primary((0.002, -0.001)); g.trace_light_paths(i); g.gather(fp, 0); g.splat_photons(fp)
        got = g.frame_error(0.2, 0.2, 1.0)
        exchange = [g.host_stats(r)["exchange_ms"] for r in range(3)]
        img = g.resolve(0.2, 0.2, 1.0)
        assert [g.host_stats(r)["exchange_ms"] for r in range(3)] == exchange      # (the resolve reused the frame_error's reduction)
        close(got, numpy_error(img, ref, mask), 1e-12)
        assert g.frame_error(0.2, 0.2, 1.0) == got


def write_inputs(evplp, d, jp_src):
    """the scene copied to d, a reference image and a mask next to it"""
    d.mkdir()
    for f in ("room.obj", "room.mtl", "room_lights.obj"):
        (d / f).write_bytes(open(os.path.join(os.path.dirname(jp_src), f), "rb").read())
    rng = np.random.default_rng(5)
    evplp.save_image(str(d / "ref.pfm"), (0.2 + 0.1 * rng.random((H, W, 3))).astype(np.float32))
    m = np.ones((H, W, 3), np.float32); m[10:22] = 0.0
    evplp.save_image(str(d / "mask.png"), m)


def render(evplp, d, jp_src, technique, conv=None, **block):
    write_inputs(evplp, d, jp_src)
    root = json.load(open(jp_src))
    if technique == "pt":
        root["pt"] = dict(rngOffset=0, numMaxIteration=7, timeLimitMs=1e9, frameMode="accumulate", outputFilename="c.pfm", statFilename="s.json",
                          useJitter=True, useStat=True, numSamplePerPixel=1, numMaxBounces=3)
        root.pop("photonfam")
        files = ("c.pfm",)
    else:
        root["photonfam"].update(numMaxIteration=7, numLightPaths=NL, numVplLightPaths=NV, radiusPercentage=0.05, misMode="balance", DoProgressive=True,
                                 deterministic=True, combinedFilename="c.pfm", weightedPhotonFilename="pm.pfm", weightedVplFilename="vpl.pfm",
                                 statFilename="s.json", run=dict(photonSplat=True))
        files = ("c.pfm", "pm.pfm", "vpl.pfm")
    root[technique].update(block)
    if conv is not None:
        root[technique]["convergence"] = conv
    jp = d / "room.json"
    json.dump(root, open(jp, "w"))
    evplp.render_json(str(jp))
    curve = json.load(open(d / "curve.json")) if conv is not None else None
    return {f: open(d / f, "rb").read() for f in files}, json.load(open(d / "s.json")), curve


CONV = {"reference": "ref.pfm", "mask": "mask.png", "everyIterations": 2, "filename": "curve.json"}


@pytest.mark.parametrize("technique, device", [("photonfam", None), ("pt", None), ("photonfam", dict(gpus=3, virtual=True, partition="iterations"))])
def test_technique_loop_checkpoints_and_unchanged_outputs(evplp, scene, tmp_path, technique, device):
    jp, _ = scene
    extra = {} if device is None else {"device": device}
    plain, st_plain, _ = render(evplp, tmp_path / "plain", jp, technique, **extra)
    imgs, st, curve = render(evplp, tmp_path / "conv", jp, technique, CONV, **extra)
    assert imgs == plain                                                 # byte-identical images
    assert st["numIterations"] == st_plain["numIterations"] == 7 and sorted(st) == sorted(st_plain)
    cps = curve["checkpoints"]
    assert [p["iteration"] for p in cps] == [2, 4, 6, 7]
    assert all(a["timeMs"] <= b["timeMs"] for a, b in zip(cps, cps[1:]))
    assert curve["pixels"] == W * H and curve["reference"] == "ref.pfm" and curve["overheadMs"] > 0
    d = tmp_path / "conv"
    ref = evplp.load_image(str(d / "ref.pfm"))
    mask, _ = evplp.decode_image(str(d / "mask.png"))
    assert curve["keptPixels"] == int(mask.any(-1).sum()) == W * (H - 12)
    img = np.ascontiguousarray(evplp.load_pfm(str(d / "c.pfm"))[::-1])        # (the written file is top-down)
    want = numpy_error(img, ref, mask)
    last = cps[-1]
    close((last["mse"], last["relMse"], last["relMseMasked"]), want, 1e-9)
    assert all(p["relMse"] > 0 for p in cps)


def test_stop_rel_mse_ends_the_run_at_its_checkpoint(evplp, scene, tmp_path):
    jp, _ = scene
    _, _, first = render(evplp, tmp_path / "first", jp, "photonfam", CONV)
    stop = [p for p in first["checkpoints"] if p["iteration"] == 4][0]["relMseMasked"] + 1e-12
    # (seeds are fixed: the second run sees the same figures and stops at the first checkpoint at or below the value -- iteration 4, unless
    # iteration 2's figure happens to be lower still)
    at = min(p["iteration"] for p in first["checkpoints"] if p["relMseMasked"] <= stop)
    assert at <= 4
    _, st, second = render(evplp, tmp_path / "second", jp, "photonfam", dict(CONV, stopRelMse=stop))
    assert [p["iteration"] for p in second["checkpoints"]] == [i for i in (2, 4) if i <= at]
    assert second["checkpoints"][-1]["iteration"] == at == st["numIterations"]
    for a, b in zip(first["checkpoints"], second["checkpoints"]):
        assert (a["mse"], a["relMse"], a["relMseMasked"]) == (b["mse"], b["relMse"], b["relMseMasked"])


def test_time_limited_run(evplp, scene, tmp_path):
    jp, _ = scene
    conv = {"reference": "ref.pfm", "everyMs": 50, "filename": "curve.json"}
    _, st, curve = render(evplp, tmp_path / "timed", jp, "photonfam", conv, timeLimitMs=300, numMaxIteration=-1)
    cps = curve["checkpoints"]
    assert len(cps) >= 3, cps                                            # at least two on the clock, and the final one
    assert cps[-1]["iteration"] == st["numIterations"]
    assert all(a["iteration"] < b["iteration"] and a["timeMs"] <= b["timeMs"] for a, b in zip(cps, cps[1:]))
    assert "keptPixels" not in curve and "relMseMasked" not in cps[-1]
