"""Device times of the temporal accumulation's three kernels beside primary_kernel and evplp_denoise's passes, from one job.

The furnished moving scene (evplp_synth_scene "conf", style "hard", 331 k triangles) at 1280 x 720, pt: frames of 2 samples, one chair moved
between them, evplp_denoise and evplp_denoise_temporal on every frame.  The frames run in a child process under `rocprofv3 --kernel-trace`
(a run of its own, under a time limit of its own); this process reads the trace and writes the median, p10 and p90 of every kernel's launches
(the first frame, which has no previous pose, left out) to profiles/temporal_times.txt.

usage: python tools/temporal_times.py [--frames N] [--tris T] [--out profiles/temporal_times.txt]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H = 1280, 720
KERNELS = ("primary_kernel", "prev_pose_kernel", "pose_snapshot_kernel", "temporal_accumulate_kernel", "denoise_prepare_kernel", "denoise_level_kernel",
           "denoise_finish_kernel")


def frames(n, tris):
    import evplp_amd as ev
    import scenes
    with tempfile.TemporaryDirectory() as d:
        jp = ev.synth_scene(d, "conf", tris, 1234, W, H, style="hard")
        sd, _ = scenes.load_obj_scene(jp)
        with ev.Context(W, H, 1, 1, 1, bvh_builder=3) as c:
            c.load_scene_json(jp); c.noise_track(True); c.temporal_enable(True)
            mesh = len(sd.meshes) // 2                           # one object in the middle of the upload order
            for f in range(n):
                if f:
                    c.transform_mesh(mesh, np.array([1, 0, 0, 0.05 * f, 0, 1, 0, 0.03 * f, 0, 0, 1, 0], np.float32)); c.refit_accel()
                c.clear_accumulators()
                jit = ev.jitter_sequence(2 * f, 2, W, H)
                for i in range(2):
                    c.primary(tuple(jit[i])); c.path_trace(sd.cam_origin, 2 * f + i, 3, accumulate=True); c.noise_fold(1)
                c.denoise(0.5)
                _, info = c.denoise_temporal(0.5)
            print("last frame:", info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_times.txt"))
    ap.add_argument("--child", action="store_true", help="the frames alone: the process rocprofv3 traces")
    a = ap.parse_args()
    if a.child:
        frames(a.frames, a.tris)
        return 0
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", "420", shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3", "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--child", "--frames", str(a.frames), "--tris", str(a.tris)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        traces = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if p.returncode != 0 or not traces:
            print(f"the traced run failed (exit {p.returncode}): {(p.stderr or p.stdout)[-800:]}", file=sys.stderr)
            return 1
        rows = list(csv.DictReader(open(traces[0])))
    lines = [f"temporal accumulation, device times per launch (us): conf / hard, {a.tris} triangles, {W} x {H}, pt, {a.frames} frames of 2 samples",
             f"{'kernel':32s} {'launches':>8s} {'median':>9s} {'p10':>9s} {'p90':>9s}"]
    for k in KERNELS:
        us = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3 for r in rows if r.get("Kernel_Name", "").startswith(k) or f" {k}" in r.get("Kernel_Name", "") or f"::{k}" in r.get("Kernel_Name", "")])
        if k in ("primary_kernel", "denoise_prepare_kernel", "denoise_level_kernel", "denoise_finish_kernel", "temporal_accumulate_kernel", "pose_snapshot_kernel"):
            us = us[len(us) // a.frames:]                       # (the first frame's launches: warm-up, and no previous pose)
        if len(us) == 0:
            lines.append(f"{k:32s} {'0':>8s}")
            continue
        lines.append(f"{k:32s} {len(us):8d} {np.median(us):9.1f} {np.percentile(us, 10):9.1f} {np.percentile(us, 90):9.1f}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
