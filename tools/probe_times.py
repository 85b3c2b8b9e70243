"""What the probe gather costs (evplp_gather_probes_device) beside what a caller had before it: the same pairs as a batch of shadow rays
through evplp_trace_occluded_device, before any shading.  One process, the furnished stand-in (evplp_synth_scene, style "hard", 331 k
triangles), 1024 light paths x 4 = 4096 record slots traced by the library, `reps` repetitions after `warmup`, HIP events on the stream
the context launches on; the batches take turns inside every repetition, so that whatever else the machine does falls on all alike.

  probes: a 16^3 and a 32^3 grid over the scene's box in grid order, and the same probes shuffled (seeded).
  pairs:  n probes x K usable records -- what the gather is asked for; it walks the pairs that pass the cosine test.
  rays:   for the comparison, the n x K shadow rays (origin pos_k, direction x - pos_k, tmin 1e-4, tmax 1 - 1e-4) built on the device with
          torch, probe-major as the caller's loop would write them, and the subset that passes the cosine test.  Building them is NOT timed:
          the figure is evplp_trace_occluded_device alone, the part of the old path that is unchanged code.

Figures: median of the repetitions (p10 - p90) in ms and M pairs/s.  A tool, not a gate.

usage: python tools/probe_times.py [--reps N] [--warmup N] [--tris N] [--paths N] [--out FILE]"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

P = 4
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_gather_times.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    Wd, Ht = 256, 144
    with tempfile.TemporaryDirectory() as d:
        sd, _ = scenes.load_obj_scene(ev.synth_scene(d, "conf", a.tris, 1234, Wd, Ht, style="hard"))
    ntri = sum(m["idx"].shape[0] for m in sd.meshes)
    verts = np.concatenate([m["verts"] for m in sd.meshes])
    lo, hi = verts.min(0).astype(np.float64), verts.max(0).astype(np.float64)
    stream = torch.cuda.Stream()
    with ev.Context(Wd, Ht, a.paths, a.paths, P) as c, torch.cuda.stream(stream):
        sd.upload(c)
        c.set_stream(stream.cuda_stream)
        c.trace_light_paths(3)
        c.synchronize()
        rec = c.download(ev.BUF_RECORDS)
        usable = np.nonzero(rec["flags"] & 1)[0]
        K = len(usable)
        info = c.accel_info()
        extent = float(np.linalg.norm(hi - lo))
        min_distance = 0.01 * extent
        say(f"scene: {ntri} triangles, builder {info['builder']}, depth {info['depth']}, stack4_entries {info['stack4_entries']}; {a.paths} paths x {P} = {a.paths * P} slots, "
            f"{K} usable, {(a.paths * P + ev.PROBE_SLICE_SLOTS - 1) // ev.PROBE_SLICE_SLOTS} slices; min_distance {min_distance:.4g}; {a.warmup} warm-up + {a.reps} repetitions; median (p10 - p90)")
        pos_k = torch.from_numpy(rec["pos"][usable].copy()).cuda()
        nrm_k = torch.from_numpy(rec["normal"][usable].copy()).cuda()
        say(f"{'batch':26s} {'pairs':>11s} {'facing':>7s} {'lit':>7s} | {'gather ms':>24s} {'M pairs/s':>10s} | {'occluded, n x K rays ms':>26s} {'M pairs/s':>10s} | {'occluded, facing rays ms':>26s} | {'gather / query':>14s}")
        for g in (16, 32):
            t = (np.arange(g) + 0.5) / g
            zz, yy, xx = np.meshgrid(t, t, t, indexing="ij")
            grid = (lo + (hi - lo) * (0.02 + 0.96 * np.stack([xx.ravel(), yy.ravel(), zz.ravel()], -1))).astype(F)
            perm = np.random.RandomState(7).permutation(len(grid))
            ref = None
            for name, x in ((f"{g}^3 grid order", grid), (f"{g}^3 shuffled", grid[perm])):
                n = len(x)
                d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
                # the caller's rays, probe-major: [n, K, 8]
                v12 = pos_k[None, :, :] - d_x[:, None, :]
                rays = torch.empty((n, K, 8), dtype=torch.float32, device="cuda")
                rays[:, :, 0:3] = pos_k[None, :, :]; rays[:, :, 3] = 1e-4; rays[:, :, 4:7] = -v12; rays[:, :, 7] = float(F(1.0) - F(0.0001))
                facing = (-(v12 * nrm_k[None, :, :]).sum(-1)) > 0
                rays = rays.reshape(-1, 8)
                rays_facing = rays[facing.reshape(-1)].contiguous()
                del v12
                out = c.gather_probes(d_x, a.paths, P, min_distance)
                occ = c.trace_occluded(rays_facing)
                c.synchronize()
                sh = out.cpu().numpy()
                lit = float(sh[:, 27].sum())
                # the same answer before anything is timed: lit pairs = unoccluded facing rays (the torch cosine test may differ from the
                # kernel's on a pair whose cosine rounds to zero: a handful of millions)
                unocc = int((occ == 0).sum().item())
                assert abs(lit - unocc) <= 1e-5 * max(unocc, 1) + 4, (lit, unocc)
                if ref is None:
                    ref = sh
                else:
                    assert sh.tobytes() == ref[perm].tobytes(), "a probe's bytes do not depend on the order of the batch"
                tg, ta, tf = [], [], []
                for rep in range(a.warmup + a.reps):
                    keep = rep >= a.warmup
                    for fn, acc in ((lambda: c.gather_probes(d_x, a.paths, P, min_distance), tg), (lambda: c.trace_occluded(rays), ta), (lambda: c.trace_occluded(rays_facing), tf)):
                        ms = timed(fn)
                        if keep:
                            acc.append(ms)
                pairs = n * K
                mg, ma, mf = spread(tg), spread(ta), spread(tf)
                say(f"{name:26s} {pairs:11d} {100.0 * rays_facing.shape[0] / pairs:6.1f}% {100.0 * lit / pairs:6.1f}% | {mg[0]:9.3f} ({mg[1]:.3f} - {mg[2]:.3f}) {pairs / mg[0] / 1e3:10.1f} | "
                    f"{ma[0]:11.3f} ({ma[1]:.3f} - {ma[2]:.3f}) {pairs / ma[0] / 1e3:10.1f} | {mf[0]:11.3f} ({mf[1]:.3f} - {mf[2]:.3f}) | {mg[0] / ma[0]:14.3f}")
                del rays, rays_facing, occ
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
