"""What tracking per-pixel noise costs (evplp_noise_*, the technique JSON's "noise" block).  One JSON line at the end of stdout.

Two BASELINE shapes on the furnished stand-in (evplp_synth_scene, style "hard", 331 k triangles), one rank:
  * config #2: 1024 x 1024, Instant Radiosity (1024 VPL paths, 3 bounces, misMode one, no photon splat);
  * config #4: 1920 x 1080, progressive photon mapping (300 000 light paths, no gather, radius 0.3 %, misMode one, DoProgressive).

(a) Per-call wall time of evplp_group_noise_fold and evplp_group_noise_estimate, host-clocked (perf_counter) from a synchronised
    device to the end of a synchronise behind the call, the two calls alternating with one rendered iteration between any two
    measurements.  Median, 10th / 90th percentile, min and max of `reps` calls each.
(b) The technique loop (evplp_render_json, numMaxIteration `iters`): ms per iteration (the stat file's time / numIterations) without a
    "noise" block, with {"batchIterations": 1} and {"batchIterations": 10} (a checkpoint every 50 iterations), and without once more
    (the spread between runs).

usage: python tools/noise_overhead.py [--reps N] [--iters N] [--configs 2,4] [--parts ab]"""
import argparse
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

import torch  # noqa: E402,F401  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

CONFIGS = {
    2: dict(W=1024, H=1024, NL=1024, NV=1024, radius=0.0, gather=True, splat=False, block=dict(
        numLightPaths=1024, numVplLightPaths=1024, radiusPercentage=0.0, misMode="one", DoProgressive=False, run={"photonSplat": False})),
    4: dict(W=1920, H=1080, NL=300000, NV=0, radius=0.003, gather=False, splat=True, block=dict(
        numLightPaths=300000, numVplLightPaths=0, radiusPercentage=0.003, misMode="one", DoProgressive=True, AlphaProgressive=0.7,
        run={"photonSplat": True})),
}
P = 4


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]
    return {"median_ms": statistics.median(xs), "p10_ms": q(0.1), "p90_ms": q(0.9), "min_ms": xs[0], "max_ms": xs[-1], "n": len(xs)}


def calls(jp, cf, reps):
    W, H, NL, NV = cf["W"], cf["H"], cf["NL"], max(cf["NV"], 1)
    sd, _ = scenes.load_obj_scene(jp)
    with ev.Group(W, H, NL, NV, P, 1, devices=[0], overlap_light_tracing=True) as g:
        g.load_scene_json(jp)
        g.set_splat_proxy()
        bsr, total, _ = g.context(0).scene_metrics()
        r = cf["radius"] * bsr
        js = ev.jitter_sequence(0, 4 * reps + 16, W, H)

        def iteration(i):
            fp = ev.frame_params(camera_pos=sd.cam_origin, mis_mode="one", pdf_mc=(NV / NL) / math.pi / (r * r) if r > 0 else 0.0,
                                 clamping_value=1.0 / total, photon_radius=r, num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P,
                                 do_accumulate=1, rng_seed=i, jitter=tuple(float(x) for x in js[i]), splat_footprint="proxy")
            g.primary(tuple(js[i])); g.trace_light_paths(i)
            if cf["gather"]:
                g.gather(fp, 0)
            if cf["splat"]:
                g.splat_photons(fp)

        g.clear_accumulators()
        g.noise_track(True)
        n = 0
        for _ in range(4):
            iteration(n); n += 1; g.noise_fold(1)
        fold, est = [], []
        for k in range(reps):
            for way in (("fold", "estimate") if k % 2 == 0 else ("estimate", "fold")):
                iteration(n); n += 1
                g.synchronize()
                t0 = time.perf_counter()
                if way == "fold":
                    g.noise_fold(1); g.synchronize()
                    fold.append((time.perf_counter() - t0) * 1e3)
                else:
                    g.noise_estimate(1.0 / n)
                    est.append((time.perf_counter() - t0) * 1e3)
                    g.noise_fold(1)
        return {"fold": spread(fold), "estimate": spread(est), "fold_bytes": 112 * W * H}


def loop_times(jp, cf, iters):
    d = os.path.dirname(jp)
    root = json.load(open(jp))
    block = dict(root["photonfam"])
    block.update(cf["block"])
    block.update({"rngOffset": 0, "numMaxIteration": iters, "timeLimitMs": 1000000000, "frameMode": "accumulate", "numMaxBounces": 3,
                  "combinedFilename": "c.pfm", "weightedPhotonFilename": "pm.pfm", "weightedVplFilename": "vpl.pfm", "statFilename": "s.json",
                  "useJitter": True, "useStat": True})
    block.pop("noise", None); block.pop("convergence", None)
    out = {}
    for name, noise in (("plain", None), ("batchIterations_1", {"batchIterations": 1, "everyIterations": 50, "filename": "noise.json"}),
                        ("batchIterations_10", {"batchIterations": 10, "everyIterations": 50, "filename": "noise.json"}), ("plain_again", None)):
        b = dict(block)
        if noise:
            b["noise"] = noise
        root["photonfam"] = b
        p = os.path.join(d, f"run_{name}.json")
        json.dump(root, open(p, "w"))
        ev.render_json(p)
        st = json.load(open(os.path.join(d, "s.json")))
        out[name] = {"ms_per_iteration": st["time"] / st["numIterations"], "iterations": st["numIterations"]}
        if noise:
            curve = json.load(open(os.path.join(d, "noise.json")))
            out[name]["checkpoints"] = len(curve["checkpoints"])
            out[name]["final_rel_mse"] = curve["checkpoints"][-1]["relMse"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--parts", default="ab")
    a = ap.parse_args()
    res = {}
    for k in (int(x) for x in a.configs.split(",")):
        cf = CONFIGS[k]
        r = {"shape": {"W": cf["W"], "H": cf["H"], "numLightPaths": cf["NL"], "numVplLightPaths": cf["NV"], "scene": "hard, 331000 triangles"}}
        with tempfile.TemporaryDirectory() as d:
            jp = ev.synth_scene(d, "conference_synth", 331000, 1234, cf["W"], cf["H"], style="hard")
            if "a" in a.parts:
                r["calls"] = calls(jp, cf, a.reps)
            if "b" in a.parts:
                r["loop"] = loop_times(jp, cf, a.iters)
        res[f"config_{k}"] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
