"""What the k-nearest-photon start radius costs (evplp_gather_surface_knn_device) beside the call it replaces as a state's first photon half,
evplp_gather_surface_progressive_device on fresh states (the yardstick).  One process, tools/surface_progressive_times.py's set-up: the
furnished stand-in (evplp_synth_scene, 331 k triangles) with config #3's records (500 000 paths x 4 = 2 M slots) traced by the library, the
1024^2 frame's own G-buffer as 1 M points, mis_mode 5, alpha = 2/3.  The bound r0 = fp->photon_radius is taken at 1 x and at 4 x of
config #3's radius 0.003 R: at 1 x few points have k photons within the bound, so most lanes stop after the first pass; 4 x is what a
caller who wants k = 64 would ask for.  HIP events on the stream the context launches on, `reps` repetitions after `warmup`; the variants
take turns inside every repetition.  Fresh states are put back OUTSIDE the timed span (a memset of 48 B a point).

  progressive           evplp_gather_surface_progressive_device, EVPLP_SURFACE_PHOTONS, fresh states: grid, compact records, one walk
  knn, k = 8 / 64       evplp_gather_surface_knn_device on fresh states: grid, compact records, the select, one walk at the selected radii
Then the kernels alone: a child process under `rocprofv3 --kernel-trace` (a run of its own) makes three calls per variant in the same
order, and the last two launches of surface_knn_select_kernel, surface_knn_photon_kernel and surface_prog_photon_kernel per variant are
averaged.  Figures: median of the repetitions (p10 - p90) in ms.  A tool, not a gate.

usage: python tools/surface_knn_times.py [--reps N] [--warmup N] [--tris N] [--paths N] [--res N] [--no-trace] [--out FILE]"""
import argparse
import csv
import glob
import math
import os
import shutil
import statistics
import subprocess
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
MULTS = (1.0, 4.0)
KS = (8, 64)
KERNELS = ("surface_knn_select_kernel", "surface_knn_photon_kernel", "surface_prog_photon_kernel")


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]       # noqa: E731
    return statistics.median(xs), q(0.1), q(0.9)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); b.synchronize()
    return a.elapsed_time(b)


def traced(a):
    """{(mult, what): {kernel: ms}} from a child under rocprofv3 --kernel-trace, or a string that says why not"""
    with tempfile.TemporaryDirectory() as d:
        cmd = [shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--kernels", "--tris", str(a.tris), "--paths", str(a.paths), "--res", str(a.res)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except (OSError, subprocess.TimeoutExpired) as e:
            return str(e)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode != 0 or not traces:
            return f"exit {p.returncode}: {(p.stderr or p.stdout)[-400:]}"
        rows = [r for r in csv.DictReader(open(traces[0])) if any(k in r.get("Kernel_Name", "") for k in KERNELS)]
    # launch order: per bound the progressive call three times, then per k the k-nearest call three times
    out, at = {}, 0
    for mult in MULTS:
        for what in ("progressive",) + KS:
            per = 3 if what == "progressive" else 6
            mine = rows[at:at + per]; at += per
            if len(mine) != per:
                return f"{len(rows)} launches traced"
            res = {}
            for k in KERNELS:
                t = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in mine if k in r["Kernel_Name"]]
                if t:
                    res[k] = statistics.mean(t[1:])
            out[(mult, what)] = res
    return out if at == len(rows) else f"{len(rows)} launches traced, {at} expected"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--paths", type=int, default=500000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--kernels", action="store_true", help="three calls per variant and stop: the child under the kernel trace")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_knn_times.txt"))
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

        def params(mult):
            return ev.frame_params(camera_pos=list(cam.origin), mis_mode=5, pdf_mc=NVPL / N / math.pi / r ** 2, photon_radius=float(F(mult * r)), num_light_paths=N,
                                   num_vpl_light_paths=NVPL, photons_per_path=P)
        c.primary((0, 0)); c.synchronize()
        planes = [c.download(b)[:H].reshape(-1, 4) for b in (ev.BUF_GBUF_POSITION, ev.BUF_GBUF_NORMAL, ev.BUF_GBUF_DIFFUSE, ev.BUF_GBUF_PHONG)]
        d_pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(planes, 1), F)).cuda()
        n = d_pts.shape[0]
        work = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
        c.trace_light_paths(0)
        c.synchronize()
        PH = ev.SURFACE_PHOTONS

        def progressive(mult):
            return c.gather_surface_progressive(d_pts, params(mult), work, alpha=ALPHA, what=PH)

        def knn(mult, k):
            return c.gather_surface_knn(d_pts, params(mult), work, k, float(F(mult * r / 64.0)), alpha=ALPHA)
        if a.kernels:
            for mult in MULTS:
                for what in ("progressive",) + KS:
                    for _ in range(3):
                        work.zero_()
                        progressive(mult) if what == "progressive" else knn(mult, what)
            c.synchronize()
            return
        flags = c.download(ev.BUF_RECORDS)["flags"]
        say(f"scene: {a.tris} triangles asked for; {W}x{H} frame as {n} points; {N} paths x {P} = {N * P} slots, {int(((flags & 2) != 0).sum())} usable photons; config #3's radius "
            f"{r:.4g}; mis_mode 5, alpha {ALPHA:.4f}, r_min = r0 / 64; {a.warmup} warm-up + {a.reps} repetitions; median (p10 - p90) ms")
        variants = []
        for mult in MULTS:
            # the same answers before anything is timed: k above every count is the progressive call, byte for byte
            work.zero_(); want = progressive(mult).clone()
            work.zero_(); got = knn(mult, 2 ** 24).clone()
            c.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))
            work.zero_(); count = c.gather_surface_progressive(d_pts, params(mult), work, alpha=1.0, what=PH)[:, 7].clone()     # n = C at alpha = 1
            c.synchronize()
            valid = float((d_pts[:, 3] != 0).sum().item())
            say(f"r0 = {mult:g} x: {int(count.double().sum().item())} photon pairs within the bound, {float(count.mean().item()):.1f} a point; " +
                ", ".join(f"C >= {k} at {100.0 * float((count >= k).sum().item()) / valid:.1f} % of the points" for k in KS))
            variants.append((f"r0 = {mult:g} x: progressive, fresh states", lambda mult=mult: progressive(mult)))
            for k in KS:
                variants.append((f"r0 = {mult:g} x: knn, k = {k}", lambda mult=mult, k=k: knn(mult, k)))
        acc = [[] for _ in variants]
        for rep in range(a.warmup + a.reps):
            for i, (_, fn) in enumerate(variants):
                work.zero_()
                ms = timed(fn)
                if rep >= a.warmup:
                    acc[i].append(ms)
        for (name, _), t in zip(variants, acc):
            m = spread(t)
            say(f"{name:44s} {m[0]:10.3f} ({m[1]:.3f} - {m[2]:.3f})")
        for mult in MULTS:
            for k in KS:
                work.zero_()
                st = knn(mult, k)
                c.synchronize()
                r2 = st[:, 3][st[:, 10].view(torch.int32) == 1]
                r0sq = float(F(mult * r) * F(mult * r))
                say(f"r0 = {mult:g} x, k = {k}: radius2 / r0sq after the call: mean {float(r2.mean().item()) / r0sq:.3f}, min {float(r2.min().item()) / r0sq:.2e}")
    if not a.no_trace:
        t = traced(a)
        if isinstance(t, str):
            say(f"kernel trace: none ({t})")
        else:
            say("kernels alone (rocprofv3 --kernel-trace in a run of its own, mean of two launches), ms:")
            for (mult, what), res in t.items():
                name = "progressive" if what == "progressive" else f"knn, k = {what}"
                say(f"r0 = {mult:g} x: {name:14s} " + ", ".join(f"{k} {v:.3f}" for k, v in res.items()))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
