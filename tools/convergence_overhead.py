"""What measuring the error of a running frame against a reference costs, on the device and the old way.  One JSON line at the end of stdout.

The shipped regime (scene/conference/conference_ours.json: 30 VPL paths, 300 000 light paths, radius 0.3 %, balance MIS, accumulate) at
1280 x 720 on the furnished stand-in (evplp_synth_scene, style "hard", 331 k triangles), one rank.

(a) Per-checkpoint wall time, host-clocked (perf_counter) after a synchronise, the two ways alternating in one process, one iteration
    rendered between any two checkpoints:
      * "device": evplp_group_frame_error -- composite, per-row reduction on the GPU, 32 bytes per row to the host;
      * "host":   evplp_group_resolve (the frame to the host), the flip to top-down rows the technique loop does, and the host
                  evplp_image_rel_mse_masked over every pixel.
    Median, 10th / 90th percentile, min and max of `reps` checkpoints each.
(b) The technique loop itself (evplp_render_json, numMaxIteration `iters`): ms per iteration (the stat file's time / numIterations) without
    a "convergence" block, with {"everyIterations": 1} (a checkpoint after every iteration) and without once more (the spread between runs).

usage: python tools/convergence_overhead.py [--reps N] [--iters N] [--parts ab]"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

W, H, NL, NV, P = 1280, 720, 300000, 30, 4


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]
    return {"median_ms": statistics.median(xs), "p10_ms": q(0.1), "p90_ms": q(0.9), "min_ms": xs[0], "max_ms": xs[-1], "n": len(xs)}


def checkpoints(jp, reps):
    sd, _ = scenes.load_obj_scene(jp)
    with ev.Group(W, H, NL, NV, P, 1, devices=[0], overlap_light_tracing=True) as g:
        g.load_scene_json(jp)
        g.set_splat_proxy()
        bsr, total, _ = g.context(0).scene_metrics()
        r = 0.003 * bsr
        js = ev.jitter_sequence(0, 2 * reps + 16, W, H)

        def iteration(i):
            fp = ev.frame_params(camera_pos=sd.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), clamping_value=1.0 / total,
                                 photon_radius=r, num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=i,
                                 jitter=tuple(float(x) for x in js[i]), splat_footprint="proxy")
            g.primary(tuple(js[i])); g.trace_light_paths(i); g.gather(fp, 0); g.splat_photons(fp)
            g.present(1.0 / (i + 1), 1.0 / (i + 1), 1.0, mask_emitter=True, gamma=True, exchange=False)

        g.clear_accumulators()
        for i in range(8):
            iteration(i)
        rng = np.random.default_rng(3)
        ref = np.ascontiguousarray(g.resolve(1.0 / 8, 1.0 / 8, 1.0)[::-1]) * (1.0 + 0.05 * rng.standard_normal((H, W, 3))).astype(np.float32)
        ref = ref.astype(np.float32)
        mask = np.full((H, W, 3), 255, np.uint8); mask[: H // 10] = 0
        g.set_error_reference(ref, mask)
        lib = ev.lib()
        dev, host, agree = [], [], []
        n = 8
        for k in range(reps):
            for way in (("device", "host") if k % 2 == 0 else ("host", "device")):
                iteration(n); n += 1
                g.synchronize()
                s = 1.0 / n
                t0 = time.perf_counter()
                if way == "device":
                    e = g.frame_error(s, s, 1.0)
                    dev.append((time.perf_counter() - t0) * 1e3)
                else:
                    img = g.resolve(s, s, 1.0)
                    top = np.ascontiguousarray(img[::-1])
                    h = lib.evplp_image_rel_mse_masked(W * H, top.ctypes.data_as(C.c_void_p), ref.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p))
                    host.append((time.perf_counter() - t0) * 1e3)
                    agree.append(abs(h - g.frame_error(s, s, 1.0)[2]) / max(abs(h), 1e-30))
        return {"device": spread(dev), "host": spread(host), "host_float_accumulator_vs_device_rel_diff_max": max(agree)}


def loop_times(jp, iters):
    d = os.path.dirname(jp)
    root = json.load(open(jp))
    block = dict(root["photonfam"])
    block.update({"rngOffset": 0, "numMaxIteration": iters, "timeLimitMs": 1000000000, "frameMode": "accumulate", "misMode": "balance",
                  "numLightPaths": NL, "numVplLightPaths": NV, "numMaxBounces": 3, "radiusPercentage": 0.003, "DoProgressive": False,
                  "combinedFilename": "c.pfm", "weightedPhotonFilename": "pm.pfm", "weightedVplFilename": "vpl.pfm", "statFilename": "s.json",
                  "useJitter": True, "useStat": True})
    block.pop("convergence", None)
    out = {}
    for name, conv in (("plain", None), ("everyIterations_1", {"reference": "ref.pfm", "mask": "mask.png", "everyIterations": 1, "filename": "curve.json"}),
                       ("plain_again", None)):
        b = dict(block)
        if conv:
            b["convergence"] = conv
        root["photonfam"] = b
        p = os.path.join(d, f"run_{name}.json")
        json.dump(root, open(p, "w"))
        ev.render_json(p)
        st = json.load(open(os.path.join(d, "s.json")))
        out[name] = {"ms_per_iteration": st["time"] / st["numIterations"], "iterations": st["numIterations"]}
        if conv:
            curve = json.load(open(os.path.join(d, "curve.json")))
            out[name]["checkpoints"] = len(curve["checkpoints"])
            out[name]["overhead_ms_per_checkpoint"] = curve["overheadMs"] / len(curve["checkpoints"])
            out[name]["final_rel_mse_masked"] = curve["checkpoints"][-1]["relMseMasked"]
        if name == "plain":        # the reference of the curve: this run's own result
            os.replace(os.path.join(d, "c.pfm"), os.path.join(d, "ref.pfm"))
            m = np.ones((H, W, 3), np.float32); m[: H // 10] = 0.0
            ev.save_image(os.path.join(d, "mask.png"), m)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--parts", default="ab")
    a = ap.parse_args()
    res = {"shape": {"W": W, "H": H, "numLightPaths": NL, "numVplLightPaths": NV, "scene": "hard, 331000 triangles"}}
    with tempfile.TemporaryDirectory() as d:
        jp = ev.synth_scene(d, "conference_synth", 331000, 1234, W, H, style="hard")
        if "a" in a.parts:
            res["checkpoint"] = checkpoints(jp, a.reps)
        if "b" in a.parts:
            res["loop"] = loop_times(jp, a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
