"""What does the variance-guided a-trous denoiser (evplp_denoise) cost and buy?  One JSON line at the end of stdout.

  * cost: one warm evplp_denoise call (variance, composite, prepare, --levels passes, finish, download) at 1280 x 720 (the shipped regime) and
    at 1024 x 1024 (config #2's size), as a host clock around the synchronised call: median and p10 - p90 over --calls calls, after two warm-up
    calls.  The inputs come from two path-traced iterations of the box room (the filter's cost does not depend on the technique).
  * gain: on the box room (--size), photonfam "ours" (VPL gather + photon splat) and pt, raw and denoised relMSE against a long run of the
    same technique (--ref-iters, other seeds) at --iters iteration counts; and the iteration count at which the raw image first reaches the
    error the denoised image has at 16 iterations (raw measured at every power of two up to --ref-iters / 2).
  * --sweep: the raw / denoised relMSE at 8 iterations for a grid of (levels, sigma_luminance, sigma_normal, sigma_position) instead.

usage: python tools/denoise_gain.py [--calls 20] [--size 128x96] [--iters 4,8,16,32,64] [--ref-iters 512] [--sweep]"""
import argparse
import itertools
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import numpy as np  # noqa: E402
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

NL, NV, P = 2048, 40, 4
JITTER = (0.002, -0.001)


def rel_mse(img, ref):
    img = img.astype(np.float64); ref = ref.astype(np.float64)
    return float((((img - ref) ** 2).sum(-1) / ((ref ** 2).sum(-1) + 0.001)).mean())


class Run:
    """one accumulating run of a technique on the box room, the noise tracker folded after every iteration"""
    def __init__(self, technique, W, H, offset=0):
        self.pt = technique == "pt"
        self.W, self.H, self.offset, self.n = W, H, offset, 0
        self.box = scenes.box_room(seed=7, n_boxes=4, tess=2, aspect=W / H)
        self.c = ev.Context(W, H, 1, 1, 1) if self.pt else ev.Context(W, H, NL, NV, P, deterministic=True)
        self.box.upload(self.c)
        self.bsr, _, _ = self.c.scene_metrics()
        self.jit = ev.jitter_sequence(offset, 4096, W, H)
        self.c.clear_accumulators(); self.c.noise_track(True)

    def advance(self, to):
        while self.n < to:
            i = self.offset + self.n
            if self.pt:
                self.c.primary(tuple(self.jit[self.n])); self.c.path_trace(self.box.cam_origin, i, 3, accumulate=True)
            else:
                r = 0.05 * self.bsr
                fp = ev.frame_params(camera_pos=self.box.cam_origin, mis_mode="balance", pdf_mc=(NV / NL) / math.pi / (r * r), photon_radius=r,
                                     num_light_paths=NL, num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=i, jitter=JITTER)
                self.c.primary(JITTER); self.c.trace_light_paths(i); self.c.gather_vpl(fp); self.c.splat_photons(fp)
            self.c.noise_fold(1)
            self.n += 1

    def raw(self):
        s = 1.0 / self.n
        return self.c.resolve(s, s, 1.0)[:self.H]

    def denoised(self, **kw):
        return self.c.denoise(1.0 / self.n, **kw)[:self.H]


def cost(W, H, calls):
    r = Run("pt", W, H)
    r.advance(2)
    for _ in range(2):
        r.denoised()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter(); r.denoised(); t.append((time.perf_counter() - t0) * 1e3)
    r.c.close()
    q = statistics.quantiles(t, n=10)
    return {"size": f"{W}x{H}", "calls": calls, "median_ms": statistics.median(t), "p10_ms": q[0], "p90_ms": q[-1]}


def gain(technique, W, H, iters, ref_iters):
    ref_run = Run(technique, W, H, offset=100000)
    ref_run.advance(ref_iters)
    ref = ref_run.raw(); ref_run.c.close()
    r = Run(technique, W, H)
    curve, raw_at = [], {}
    for n in sorted(set(iters) | {16}):
        r.advance(n)
        e = {"iterations": n, "raw": rel_mse(r.raw(), ref), "denoised": rel_mse(r.denoised(), ref)}
        raw_at[n] = e["raw"]
        if n in iters:
            curve.append(e)
        if n == 16:
            target = e["denoised"]
    n, reach = 16, None
    while n <= ref_iters // 2:
        r.advance(n)
        raw_at[n] = rel_mse(r.raw(), ref)
        if raw_at[n] <= target:
            reach = n
            break
        n *= 2
    r.c.close()
    return {"technique": technique, "curve": curve, "denoised_at_16": target, "raw_reaches_it_at": reach,
            "raw_by_iterations": {str(k): v for k, v in sorted(raw_at.items())}}


def sweep(technique, W, H, ref_iters):
    ref_run = Run(technique, W, H, offset=100000)
    ref_run.advance(ref_iters)
    ref = ref_run.raw(); ref_run.c.close()
    r = Run(technique, W, H)
    r.advance(8)
    raw = rel_mse(r.raw(), ref)
    rows = []
    for lv, sl, sn, sx in itertools.product((2, 3, 4, 5), (0.5, 1.0, 2.0, 4.0), (32.0, 128.0), (0.002, 0.01, 0.05)):
        rows.append({"levels": lv, "sigma_luminance": sl, "sigma_normal": sn, "sigma_position": sx,
                     "ratio": rel_mse(r.denoised(levels=lv, sigma_luminance=sl, sigma_normal=sn, sigma_position=sx), ref) / raw})
    r.c.close()
    rows.sort(key=lambda x: x["ratio"])
    return {"technique": technique, "raw_at_8": raw, "best": rows[:8], "defaults": [x for x in rows if (x["levels"], x["sigma_luminance"], x["sigma_normal"], x["sigma_position"]) == (5, 4.0, 128.0, 0.01)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", default="128x96")
    ap.add_argument("--iters", default="4,8,16,32,64")
    ap.add_argument("--ref-iters", type=int, default=512)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    W, H = (int(v) for v in a.size.split("x"))
    if a.sweep:
        out = {"sweep": [sweep(t, W, H, a.ref_iters) for t in ("photonfam", "pt")]}
    else:
        out = {"cost": [cost(1280, 720, a.calls), cost(1024, 1024, a.calls)],
               "gain": [gain(t, W, H, [int(v) for v in a.iters.split(",")], a.ref_iters) for t in ("photonfam", "pt")], "size": f"{W}x{H}"}
    for k, v in out.items():
        print(k, json.dumps(v, indent=1), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
