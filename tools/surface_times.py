"""What the surface gather costs (evplp_gather_surface_device) beside the frame's own passes on the same pairs.  One process, the furnished
stand-in (evplp_synth_scene, 331 k triangles) with config #3's records (500 000 paths x 4 = 2 M slots, r = 0.003 R, the first 1 024 paths
x 4 = 4 096 slots as VPLs) traced by the library, and the 1024^2 frame's own G-buffer as 1 M points.  HIP events on the stream the context
launches on, `reps` repetitions after `warmup`; the variants take turns inside every repetition, so that whatever else the machine does
falls on all alike.

  photons, 1 M points      the grid build (cells and keys, the radix sort, bucket starts, compact records) and the query, in frame order
  photons, shuffled        the same points in a seeded random order
  photons, 64 points       the grid build with next to no query: what a call pays before its first point
  splat_photons(IDEAL)     the parent's pass on the same pairs: bins by projected tile, one wave per tile
  VPL half, 1 M points     4 096 slots, 16 slices
  gather_lvc, full window  the parent's per-lane walk and shading on the same pairs (1 024 of 1 024 paths), one wave per tile, no partial sums
  both halves, 4 096       a small batch: every 256th point

--kernels runs the photon half twice and stops: for a kernel trace of the grid build (cell, sort, bucket, compact) and the query.
Figures: median of the repetitions (p10 - p90) in ms.  A tool, not a gate.

usage: python tools/surface_times.py [--reps N] [--warmup N] [--tris N] [--paths N] [--kernels] [--out FILE]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_gather_times.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    W = H = a.res
    N = a.paths
    stream = torch.cuda.Stream()
    # (gather_lvc takes its window out of ALL of a context's paths: a second context of 1 024 paths holds the VPL slots alone)
    with tempfile.TemporaryDirectory() as d, ev.Context(W, H, N, NVPL, P) as c, ev.Context(W, H, NVPL, NVPL, P) as c_lvc, torch.cuda.stream(stream):
        jp = ev.synth_scene(d, "conf", a.tris, 1234, W, H)
        for ctx in (c, c_lvc):
            ctx.load_scene_json(jp)
            ctx.set_stream(stream.cuda_stream)
        cam = c.camera(); bsr, _, _ = c.scene_metrics(); r = 0.003 * bsr
        kw = dict(camera_pos=list(cam.origin), mis_mode="balance", pdf_mc=NVPL / N / math.pi / r ** 2, photon_radius=r, num_light_paths=N,
                  num_vpl_light_paths=NVPL, photons_per_path=P)
        fp = ev.frame_params(**kw)
        fp_lvc = ev.frame_params(**dict(kw, num_light_paths=NVPL))          # a window of all of the first 1 024 paths
        c.primary((0, 0)); c.trace_light_paths(0)
        c_lvc.primary((0, 0)); c_lvc.trace_light_paths(0)
        c.synchronize(); c_lvc.synchronize()
        assert c_lvc.download(ev.BUF_RECORDS).tobytes() == c.download(ev.BUF_RECORDS)[:NVPL * P].tobytes(), "the first 1 024 paths are the same records"
        planes = [c.download(b)[:H].reshape(-1, 4) for b in (ev.BUF_GBUF_POSITION, ev.BUF_GBUF_NORMAL, ev.BUF_GBUF_DIFFUSE, ev.BUF_GBUF_PHONG)]
        pts = np.ascontiguousarray(np.concatenate(planes, 1), F)
        n = len(pts)
        perm = np.random.RandomState(7).permutation(n)
        d_pts = torch.from_numpy(pts).cuda()
        d_shuf = torch.from_numpy(np.ascontiguousarray(pts[perm])).cuda()
        d_tiny = d_pts[:64].contiguous()
        d_small = d_pts[::256].contiguous()
        flags = c.download(ev.BUF_RECORDS)["flags"]
        if a.kernels:
            for _ in range(2):
                c.gather_surface(d_pts, fp, what=ev.SURFACE_PHOTONS)
            c.synchronize()
            return
        # the same answers before anything is timed
        got = c.gather_surface(d_pts, fp); shuf = c.gather_surface(d_shuf, fp, what=ev.SURFACE_PHOTONS)
        c.splat_photons(fp, clear=True); c.synchronize()
        pairs = c.pass_stats(ev.PASS_SPLAT)["pairs"]
        c.clear_accumulators(); c.gather_vpl(fp); c.synchronize()
        shaded = c.pass_stats(ev.PASS_GATHER_VPL)["shaded"]
        g = got.cpu().numpy(); valid = pts[:, 3] != 0
        assert g[:, 4:].tobytes() == shuf.cpu().numpy()[np.argsort(perm)][:, 4:].tobytes(), "a point's photon bytes do not depend on the order of the batch"
        # (splat_photons is built with contraction: its radius test fuses the squares, and a few pairs in ten million on the sphere's skin fall
        # on the other side; this unit's test has the oracle's roundings -- tests/test_gpu_surface.py counts it exactly)
        inside = int(g[:, 7].astype(np.float64).sum())
        assert valid.all() and abs(inside - pairs) <= 1e-5 * pairs, (inside, pairs)
        lit = int(g[:, 3].astype(np.float64).sum())
        assert lit == shaded, (lit, shaded)
        say(f"scene: {a.tris} triangles asked for; {W}x{H} frame, {int(valid.sum())} of {n} points valid; {N} paths x {P} = {N * P} slots, {int(((flags & 2) != 0).sum())} usable photons, "
            f"radius {r:.4g}; {NVPL * P} VPL slots, {int(((flags[:NVPL * P] & 1) != 0).sum())} usable; {inside} photon pairs (splat_photons: {pairs}), {shaded} lit VPL pairs; "
            f"{a.warmup} warm-up + {a.reps} repetitions; median (p10 - p90) ms")
        variants = [
            ("photons, 1 M points", lambda: c.gather_surface(d_pts, fp, what=ev.SURFACE_PHOTONS)),
            ("photons, shuffled", lambda: c.gather_surface(d_shuf, fp, what=ev.SURFACE_PHOTONS)),
            ("photons, 64 points (the grid build)", lambda: c.gather_surface(d_tiny, fp, what=ev.SURFACE_PHOTONS)),
            ("splat_photons(IDEAL)", lambda: c.splat_photons(fp, clear=True)),
            ("VPL half, 1 M points", lambda: c.gather_surface(d_pts, fp, what=ev.SURFACE_VPL)),
            ("VPL half, shuffled", lambda: c.gather_surface(d_shuf, fp, what=ev.SURFACE_VPL)),
            ("gather_lvc, full window", lambda: c_lvc.gather_lvc(fp_lvc)),
            (f"both halves, {len(d_small)} points", lambda: c.gather_surface(d_small, fp)),
        ]
        acc = [[] for _ in variants]
        for rep in range(a.warmup + a.reps):
            for k, (_, fn) in enumerate(variants):
                ms = timed(fn)
                if rep >= a.warmup:
                    acc[k].append(ms)
        for (name, _), t in zip(variants, acc):
            m = spread(t)
            say(f"{name:38s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
