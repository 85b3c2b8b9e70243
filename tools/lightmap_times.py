"""What baking a lightmap costs (evplp_lightmap_samples_device, evplp_surface_points_device, evplp_bake_lightmap_device) beside the surface
gather on the same points (evplp_gather_surface_device: the call the bake chains, and all there was before).  One process, the furnished
stand-in (evplp_synth_scene, 331 k triangles) with config #3's records (500 000 paths x 4 = 2 M slots, r = 0.003 R, the first 1 024 paths
x 4 = 4 096 slots as VPLs) traced by the library; the atlas is the whole scene (mesh = -1) with its own texcoords, at 256^2 and 1024^2 texels
and 1 and 2 samples per axis.  HIP events on the stream the context launches on, `reps` repetitions after `warmup`; the variants of an atlas
take turns inside every repetition, so that whatever else the machine does falls on all alike.

  raster           evplp_lightmap_samples_device over the atlas: per band the count, the scan, one 4-byte read-back (the host waits there: the
                   time includes it), the fill and the raster kernel; "per band" is that time divided by the number of bands
  points           evplp_surface_points_device on the atlas's samples (1 M hits at 1024^2, S = 1)
  gather           evplp_gather_surface_device on those points, both halves: the parent's own call
  bake, gutter 0   the whole chain with the resolve
  bake, gutter 2   ... and two gutter passes; "gutter" is the difference of the two inside each repetition, per pass

--kernels runs one bake of the 1024^2, S = 2 atlas with gutter 2 twice and stops: for a kernel trace (resolve and gutter by kernel).
Figures: median of the repetitions (p10 - p90) in ms.  A tool, not a gate.

usage: python tools/lightmap_times.py [--reps N] [--warmup N] [--tris N] [--paths N] [--kernels] [--out FILE]"""
import argparse
import math
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402

P, NVPL = 4, 1024
ATLASES = ((256, 1), (256, 2), (1024, 1), (1024, 2))


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]       # noqa: E731
    return statistics.median(xs), q(0.1), q(0.9)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--paths", type=int, default=500000)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_times.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    N = a.paths
    stream = torch.cuda.Stream()
    with tempfile.TemporaryDirectory() as d, ev.Context(64, 64, N, NVPL, P) as c, torch.cuda.stream(stream):
        jp = ev.synth_scene(d, "conf", a.tris, 1234, 64, 64)
        c.load_scene_json(jp)
        c.set_stream(stream.cuda_stream)
        cam = c.camera(); bsr, _, _ = c.scene_metrics(); r = 0.003 * bsr
        fp = ev.frame_params(camera_pos=list(cam.origin), mis_mode="balance", pdf_mc=NVPL / N / math.pi / r ** 2, photon_radius=r, num_light_paths=N,
                             num_vpl_light_paths=NVPL, photons_per_path=P)
        c.trace_light_paths(0)
        c.synchronize()
        if a.kernels:
            for _ in range(2):
                c.bake_lightmap_device(fp, 1024, 1024, 2, gutter=2)
            c.synchronize()
            return
        flags = c.download(ev.BUF_RECORDS)["flags"]
        say(f"scene: {a.tris} triangles asked for; {N} paths x {P} = {N * P} slots, {int(((flags & 2) != 0).sum())} usable photons, radius {r:.4g}; {NVPL * P} VPL slots, "
            f"{int(((flags[:NVPL * P] & 1) != 0).sum())} usable; mesh = -1, the scene's own texcoords; {a.warmup} warm-up + {a.reps} repetitions; median (p10 - p90) ms")
        for res, S in ATLASES:
            n = res * res * S * S
            bands = -(-res // max(1, ev.LIGHTMAP_CHUNK // (res * S * S)))
            hits = c.lightmap_samples_device(res, res, S)
            pts = c.surface_points(hits)
            light = c.gather_surface(pts, fp)
            baked = c.bake_lightmap_device(fp, res, res, S, gutter=2)
            c.synchronize()
            covered = int((hits[:, 3] >= 0).sum().item())
            cov = baked[..., 3]
            # the same answers before anything is timed: a fully covered texel's VPL sum is the mean of its samples' results
            full = (cov == 1.0).reshape(-1)
            mean = light[:, :3].reshape(res * res, S * S, 3).double().mean(1)[full]
            assert full.any() and torch.allclose(baked[..., :3].reshape(-1, 3)[full].double(), mean, rtol=1e-5, atol=1e-7)
            say(f"atlas {res} x {res}, S = {S}: {n} samples in {bands} bands, {covered} covered ({100.0 * covered / n:.1f} %), {int((cov > 0).sum().item())} texels covered, "
                f"{int((cov < 0).sum().item())} filled by the gutter")
            variants = [
                ("raster", lambda: c.lightmap_samples_device(res, res, S)),
                ("points", lambda: c.surface_points(hits)),
                ("gather (evplp_gather_surface_device)", lambda: c.gather_surface(pts, fp)),
                ("bake, gutter 0", lambda: c.bake_lightmap_device(fp, res, res, S, gutter=0)),
                ("bake, gutter 2", lambda: c.bake_lightmap_device(fp, res, res, S, gutter=2)),
            ]
            acc = [[] for _ in variants]
            for rep in range(a.warmup + a.reps):
                for k, (_, fn) in enumerate(variants):
                    ms = timed(fn)
                    if rep >= a.warmup:
                        acc[k].append(ms)
            for (name, _), t in zip(variants, acc):
                m = spread(t)
                say(f"  {name:38s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
            m = spread([x / bands for x in acc[0]])
            say(f"  {'raster per band':38s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
            m = spread([(g2 - g0) / 2.0 for g0, g2 in zip(acc[3], acc[4])])
            say(f"  {'gutter, per pass (difference)':38s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
            m = spread([b - (ra + po + ga) for ra, po, ga, b in zip(acc[0], acc[1], acc[2], acc[3])])
            say(f"  {'bake 0 - (raster + points + gather)':38s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
