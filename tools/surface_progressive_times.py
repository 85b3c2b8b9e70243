"""What one iteration of the progressive surface gather costs (evplp_gather_surface_progressive_device) beside the plain call on the same
points and records (evplp_gather_surface_device: the yardstick).  One process, the furnished stand-in (evplp_synth_scene, 331 k triangles)
with config #3's records (500 000 paths x 4 = 2 M slots, r = 0.003 R, the first 1 024 paths x 4 = 4 096 slots as VPLs) traced by the
library, and the 1024^2 frame's own G-buffer as 1 M points: tools/surface_times.py's set-up, in mis_mode 5.  HIP events on the stream the
context launches on, `reps` repetitions after `warmup`; the variants take turns inside every repetition, so that whatever else the machine
does falls on all alike.  The states a timed call starts from are put back OUTSIDE the timed span (a device-to-device copy of 48 B a point).

  plain                 evplp_gather_surface_device
  iteration 1           fresh states: every radius is the call's
  iteration 16          states that went through 15 iterations at alpha = 2/3 (light paths retraced with seeds 1 .. 15), then the timed
                        one on seed 0's records -- the records of the two rows above
each for the photon half alone and for both halves.  --kernels runs the plain photon half and the progressive one (iterations 1 and 2)
twice each and stops: for a kernel trace.  Figures: median of the repetitions (p10 - p90) in ms.  A tool, not a gate.

usage: python tools/surface_progressive_times.py [--reps N] [--warmup N] [--tris N] [--paths N] [--res N] [--kernels] [--out FILE]"""
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
F = np.float32
ALPHA = 2.0 / 3.0


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
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_progressive_times.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    W = H = a.res
    N = a.paths
    stream = torch.cuda.Stream()
    with tempfile.TemporaryDirectory() as d, ev.Context(W, H, N, NVPL, P) as c, torch.cuda.stream(stream):
        c.load_scene_json(ev.synth_scene(d, "conf", a.tris, 1234, W, H))
        c.set_stream(stream.cuda_stream)
        cam = c.camera(); bsr, _, _ = c.scene_metrics(); r = 0.003 * bsr
        fp = ev.frame_params(camera_pos=list(cam.origin), mis_mode=5, pdf_mc=NVPL / N / math.pi / r ** 2, photon_radius=r, num_light_paths=N,
                             num_vpl_light_paths=NVPL, photons_per_path=P)
        c.primary((0, 0)); c.synchronize()
        planes = [c.download(b)[:H].reshape(-1, 4) for b in (ev.BUF_GBUF_POSITION, ev.BUF_GBUF_NORMAL, ev.BUF_GBUF_DIFFUSE, ev.BUF_GBUF_PHONG)]
        d_pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(planes, 1), F)).cuda()
        n = d_pts.shape[0]
        fresh = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
        work = {k: torch.zeros_like(fresh) for k in ("p1", "p16", "b1", "b16")}
        if a.kernels:
            c.trace_light_paths(0)
            for _ in range(2):
                c.gather_surface(d_pts, fp, what=ev.SURFACE_PHOTONS)
                c.gather_surface_progressive(d_pts, fp, work["p1"], alpha=ALPHA, what=ev.SURFACE_PHOTONS)
            c.synchronize()
            return
        # fifteen iterations, each on its own light paths: the photon half alone decides the radii, so one run serves both rows
        late = torch.zeros_like(fresh)
        for it in range(1, 16):
            c.trace_light_paths(it)
            c.gather_surface_progressive(d_pts, fp, late, alpha=ALPHA, what=ev.SURFACE_PHOTONS)
        c.trace_light_paths(0)
        c.synchronize()
        # the same answers before anything is timed: iteration 1 at alpha = 1 keeps exactly the photons the plain call counts
        plain = c.gather_surface(d_pts, fp)
        one = c.gather_surface_progressive(d_pts, fp, torch.zeros_like(fresh), alpha=1.0)
        c.synchronize()
        assert torch.equal(one[:, 7], plain[:, 7]) and torch.equal(one[:, 4:7], plain[:, :3]) and torch.equal(one[:, 8], plain[:, 3])
        st = late.cpu().numpy().view(ev.SURFACE_STATE_DTYPE).reshape(-1)
        live = st["pm_calls"] > 0
        r0sq = float(F(r) * F(r))
        flags = c.download(ev.BUF_RECORDS)["flags"]
        say(f"scene: {a.tris} triangles asked for; {W}x{H} frame as {n} points, {int(live.sum())} valid; {N} paths x {P} = {N * P} slots, {int(((flags & 2) != 0).sum())} usable photons, "
            f"radius {r:.4g}; {NVPL * P} VPL slots; mis_mode 5, alpha {ALPHA:.4f}; {int(plain[:, 7].double().sum().item())} photon pairs at the call's radius; after 15 iterations "
            f"radius2 / r0sq: mean {float(st['radius2'][live].mean() / r0sq):.3f}, min {float(st['radius2'][live].min() / r0sq):.3f}; {a.warmup} warm-up + {a.reps} repetitions; median (p10 - p90) ms")
        PH, BOTH = ev.SURFACE_PHOTONS, ev.SURFACE_VPL | ev.SURFACE_PHOTONS
        variants = [
            ("photon half: plain", None, None, lambda: c.gather_surface(d_pts, fp, what=PH)),
            ("photon half: iteration 1", "p1", fresh, lambda: c.gather_surface_progressive(d_pts, fp, work["p1"], alpha=ALPHA, what=PH)),
            ("photon half: iteration 16", "p16", late, lambda: c.gather_surface_progressive(d_pts, fp, work["p16"], alpha=ALPHA, what=PH)),
            ("both halves: plain", None, None, lambda: c.gather_surface(d_pts, fp, what=BOTH)),
            ("both halves: iteration 1", "b1", fresh, lambda: c.gather_surface_progressive(d_pts, fp, work["b1"], alpha=ALPHA, what=BOTH)),
            ("both halves: iteration 16", "b16", late, lambda: c.gather_surface_progressive(d_pts, fp, work["b16"], alpha=ALPHA, what=BOTH)),
        ]
        acc = [[] for _ in variants]
        for rep in range(a.warmup + a.reps):
            for k, (_, slot, start, fn) in enumerate(variants):
                if slot:
                    work[slot].copy_(start)
                ms = timed(fn)
                if rep >= a.warmup:
                    acc[k].append(ms)
        for (name, _, _, _), t in zip(variants, acc):
            m = spread(t)
            say(f"{name:38s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
        say(f"state traffic of one photon half: {n} points x 96 B = {n * 96 / 1e6:.1f} MB")
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
