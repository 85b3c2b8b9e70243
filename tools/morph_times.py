"""Morphing meshes by targets (evplp_morph_mesh) beside handing the same blended positions to evplp_update_mesh -- what a caller did before
there were targets --, each followed by evplp_refit_accel.  One process, the furnished stand-in (evplp_synth_scene, style "hard", 331 k
triangles), every chair under T = 4 and then T = 64 targets (swellings and leans that are functions of the rest position), the weights
alternating between two sets so that every refit really moves the chairs.  `reps` repetitions, median with p10 - p90:

  - the refit's HIP-event time and its four stages (evplp_refit_info, evplp_debug_accel(6) under evplp_profile_kernels), in a loop of its own
    with the stage events on.  In a refit that only morphs, the first stage, "vertices", is two small copies (4 B x T per mesh and a 32 B
    descriptor per mesh) and refit_morph_kernel, so the stage is an upper bound of the kernel's time; the bytes per second below divide the
    bytes the kernel must move -- per triangle T x 36 B of deltas and 36 B of rest pose read and 36 B written, that is
    (T x 12 + 12 + 12) B per corner -- by that stage's time;
  - the host's wall time of the move calls and of the refit call, with the stage events off;
  - for the upload rows the host's blend itself (numpy fp32, the restatement of morph_point) is timed apart: a caller pays it too.

usage: python tools/morph_times.py [--reps N] [--tris N] [--res N] [--targets 4,64]"""
import argparse
import os
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

from refit_times import chair_meshes, context, spread  # noqa: E402
from skin_times import STAGES, loop  # noqa: E402

F = np.float32


def targets_of(v, T):
    """T targets of a chair: target k swells it about its axis, more with the height, and leans it along axis k % 2"""
    lo, hi = v.min(0), v.max(0)
    ctr = F(0.5) * (lo + hi)
    t = ((v[:, 2] - lo[2]) / max(float(hi[2] - lo[2]), 1e-3)).astype(F)
    d = np.empty((T,) + v.shape, F)
    for k in range(T):
        d[k] = (v - ctr) * F(0.04 * (1 + k % 4) / T * 4) * t[:, None]
        d[k][:, 2] = 0
        d[k][:, k % 2] += t * F(0.02 * (1 + k % 3) / T * 4)
    return d


def blend(p, d, w):
    out = p.copy()
    for k in range(len(w)):
        out = out + w[k] * d[k]
    return out


def report(c, sd, meshes, move, reps, how, T=None):
    tris = sum(sd.meshes[m]["idx"].shape[0] for m in meshes)
    print(f"every chair by {how}: {len(meshes)} mesh(es), {tris} triangles moved")
    ev_ms, st, _, _ = loop(c, meshes, move, reps, True)
    print(f"      device, whole refit (stage events on)        ms {spread(ev_ms)}")
    for k, n in enumerate(STAGES):
        print(f"      device, {n:36s} ms {spread(st[:, k].tolist())}")
    if T is not None:
        must = 3 * tris * (T * 12 + 12 + 12)
        ms = float(np.median(st[:, 0]))
        print(f"      refit_morph_kernel: {must / 1e6:.1f} MB to move (T x 12 B + 12 B read + 12 B written per corner); within the vertices stage "
              f"({ms:.4f} ms, the two small copies included) that is at least {must / (ms * 1e-3) / 1e9:.0f} GB/s")
    ev_ms, _, t_move, t_refit = loop(c, meshes, move, reps, False)
    print(f"      device, whole refit (stage events off)       ms {spread(ev_ms)}")
    print(f"      host, {how + ' calls':38s} ms {spread(t_move)}")
    print(f"      host, refit_accel call                       ms {spread(t_refit)}")
    print(f"      host, both                                   ms {spread([a + b for a, b in zip(t_move, t_refit)])}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--targets", default="4,64")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="evplp_morph_") as d:
        sd, _ = scenes.load_obj_scene(ev.synth_scene(d, "conf", a.tris, 1234, a.res, a.res, style="hard"))
    ntri = sum(m["idx"].shape[0] for m in sd.meshes)
    chairs = chair_meshes(sd)
    print(f"library: {ev.LIB_PATH}")
    print(f"scene: {ntri} triangles in {len(sd.meshes)} meshes, {len(chairs)} chairs found; {a.reps} repetitions; median (p10 - p90)")
    c = context(sd, a.res, ev.BVH_SAH)
    for T in [int(t) for t in a.targets.split(",")]:
        rng = np.random.default_rng(T)
        sets = [rng.uniform(-0.25, 1.25, T).astype(F) for _ in range(2)]
        targets = {m: targets_of(sd.meshes[m]["verts"], T) for m in chairs}
        print(f"---- T = {T} targets per chair")
        t0 = time.perf_counter()
        blended = {m: [blend(sd.meshes[m]["verts"], targets[m], w) for w in sets] for m in chairs}
        t1 = time.perf_counter()
        print(f"      host, the blend itself in numpy fp32 (what the upload path's caller also pays), all chairs, per weight set: {(t1 - t0) * 1e3 / 2:.3f} ms")
        for m in chairs:
            assert blended[m][0].tobytes() == ev.morph_points(sd.meshes[m]["verts"], targets[m], sets[0]).tobytes()
        report(c, sd, chairs, lambda m, k: c.update_mesh(m, blended[m][k]), a.reps, "update_mesh")
        for m in chairs:
            c.update_mesh(m, sd.meshes[m]["verts"])
        c.refit_accel()
        for m in chairs:
            c.set_mesh_morph(m, targets[m])
        report(c, sd, chairs, lambda m, k: c.morph_mesh(m, sets[k]), a.reps, "morph_mesh", T)
        for m in chairs:
            c.morph_mesh(m, None)
        c.refit_accel()
        for m in chairs:
            c.set_mesh_morph(m, None)
    c.close()


if __name__ == "__main__":
    main()
