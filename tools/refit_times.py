"""What a moving scene costs (evplp_update_mesh + evplp_refit_accel) beside a rebuild.  One process, the furnished stand-in
(evplp_synth_scene, style "hard", 331 k triangles), `reps` repetitions each, median with p10 - p90.

  (1) evplp_refit_accel after moving (a) one chair's mesh, (b) every mesh by a small translation: HIP events on the context's stream
      (evplp_refit_info; the stages -- vertex upload, leaf operands, boxes with the number of launches, four-wide nodes -- from
      evplp_debug_accel(6) under evplp_profile_kernels) and the host's wall time of the update calls and of the refit call.
  (2) evplp_build_accel with the default SAH builder and with the device LBVH: accel_info()["build_ms"] and the wall time of the call.
  (3) the config-#2 gather (tools/quick_bench.py's pass: 1024 x 1024, 1024 VPL paths, misMode one) over three trees of the SAME moved scene
      (b): the refitted SAH tree, a rebuilt SAH tree, a rebuilt device LBVH.
  (4) the same for a large motion: every chair displaced by a metre in a seeded direction -- what the topology's ageing costs.
  (5) evplp_accel_quality on the SAH tree: HIP events on the context's stream (evplp_debug_accel(7)) and the host's wall time of the call.
  (6) does the figure track the time?  For the motions of (3) and (4) and three larger ones -- neighbouring chairs swapped (they have passed
      through each other), the two rows of chairs swapped across the room, every chair at another chair's place (seeded) -- the SAH cost
      (evplp_accel_quality) of the refitted SAH tree and of a rebuilt SAH tree of the same moved scene, and beside it the config-#2 gather
      time of each.

  (7) --transform: the motions of (1) -- one chair, every mesh -- by upload (evplp_update_mesh) and by matrix (evplp_transform_mesh), each
      followed by evplp_refit_accel: the host's wall time of the move calls and of the refit call, and the refit's HIP-event time.
      --package-root DIR imports evplp_amd (and its library) from another checkout, for an A/B against it in alternating processes; a
      checkout without evplp_transform_mesh prints the upload rows alone.

  (8) --rotate: tree rotations (evplp_set_refit_rotations, evplp_optimize_accel).  For the five motions of (6): the refitted SAH tree without
      and with 1, 2 and 4 rotation passes -- rotations taken, SAH cost, the config-#2 gather, and the refit's HIP-event and host time with
      the passes on -- beside a rebuilt SAH tree and a PLOC rebuild of the same moved scene, all in one process, the gathers of one motion
      taking turns; then evplp_optimize_accel over fresh device-LBVH and PLOC trees (its call time includes the tree's plan, made once).

usage: python tools/refit_times.py [--reps N] [--tris N] [--res N] [--quality-only | --transform | --rotate] [--package-root DIR]"""
import argparse
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1]) if "--package-root" in sys.argv[1:-1] else ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

P, NL = 4, 1024
GPU_BUILDER = ev.BVH_LBVH_GPU
F = np.float32
# synth_scene.cpp places the chairs here (style "hard"); every chair is one object = one mesh
CHAIRS = [(0.9 + 1.37 * i, y) for i in range(7) for y in (-1.9, 3.9)] + [(-1.0, 1.0), (11.0, 1.0)]


def spread(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]
    return "%9.3f  (%.3f - %.3f)" % (statistics.median(xs), q(0.1), q(0.9))


def chair_meshes(sd):
    out = []
    for k, m in enumerate(sd.meshes):
        lo, hi = m["verts"].min(0), m["verts"].max(0)
        c = 0.5 * (lo + hi)
        if k != sd.light_mesh and lo[2] < 0.1 and 1.0 < hi[2] < 1.9 and max(hi[0] - lo[0], hi[1] - lo[1]) < 1.7 and any(math.hypot(c[0] - x, c[1] - y) < 0.5 for x, y in CHAIRS):
            out.append(k)
    return out


def context(sd, res, builder, verts=None):
    c = ev.Context(res, res, NL, NL, P, bvh_builder=builder)
    if verts is None:
        sd.upload(c)
    else:
        moved = scenes.SceneData.__new__(scenes.SceneData)
        moved.__dict__.update(sd.__dict__)
        moved.meshes = [dict(m, verts=verts[k]) for k, m in enumerate(sd.meshes)]
        moved.upload(c)
    return c


def time_refits(c, sd, meshes, sets, reps, name):
    """alternates between the vertex sets; every refit really moves the meshes"""
    c.profile_kernels(True)
    ev_ms, stages, t_update, t_refit = [], [], [], []
    for r in range(reps + 2):
        c.synchronize()
        t0 = time.perf_counter()
        for m in meshes:
            c.update_mesh(m, sets[r % 2][m])
        t1 = time.perf_counter()
        c.refit_accel()
        t2 = time.perf_counter()
        info = c.refit_info()
        if r >= 2:                                                  # (the first builds the plan, the second warms the kernels)
            ev_ms.append(info["last_refit_ms"]); stages.append(c.debug_accel(6).copy()); t_update.append((t1 - t0) * 1e3); t_refit.append((t2 - t1) * 1e3)
    st = np.array(stages)
    tris = sum(sd.meshes[m]["idx"].shape[0] for m in meshes)
    print(f"(1) refit, {name}: {len(meshes)} mesh(es), {tris} triangles moved, {info['levels']} box launches")
    print(f"      device, whole refit          ms {spread(ev_ms)}")
    for k, n in enumerate(("vertex upload + scatter", "leaf operands", "boxes, all levels", "four-wide nodes")):
        print(f"      device, {n:24s} ms {spread(st[:, k].tolist())}")
    print(f"      host, update_mesh calls      ms {spread(t_update)}")
    print(f"      host, refit_accel call       ms {spread(t_refit)}")
    c.profile_kernels(False)
    return statistics.median(ev_ms), statistics.median(t_refit)


def time_moves(c, sd, meshes, sets, reps, name):
    """(7): sets = two vertex sets (by upload) or two matrices (by transform), alternated so that every refit really moves the meshes"""
    by_matrix = not isinstance(sets[0], list)
    ev_ms, t_move, t_refit = [], [], []
    for r in range(reps + 2):
        c.synchronize()
        t0 = time.perf_counter()
        for m in meshes:
            c.transform_mesh(m, sets[r % 2]) if by_matrix else c.update_mesh(m, sets[r % 2][m])
        t1 = time.perf_counter()
        c.refit_accel()
        t2 = time.perf_counter()
        info = c.refit_info()
        if r >= 2:                                                  # (the first builds the plan and the rest pose, the second warms the kernels)
            ev_ms.append(info["last_refit_ms"]); t_move.append((t1 - t0) * 1e3); t_refit.append((t2 - t1) * 1e3)
    tris = sum(sd.meshes[m]["idx"].shape[0] for m in meshes)
    how = "transform_mesh" if by_matrix else "update_mesh"
    print(f"(7) {name} by {how}: {len(meshes)} mesh(es), {tris} triangles moved")
    print(f"      host, {how + ' calls':22s} ms {spread(t_move)}")
    print(f"      host, refit_accel call       ms {spread(t_refit)}")
    print(f"      device, whole refit          ms {spread(ev_ms)}")


def time_builds(c, reps, name):
    ms, wall = [], []
    for _ in range(reps):
        c.synchronize()
        t0 = time.perf_counter(); c.build_accel(); c.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(c.accel_info()["build_ms"])
    print(f"(2) evplp_build_accel, {name}: build_ms {spread(ms)}   wall ms {spread(wall)}   {c.accel_info()}")
    return statistics.median(wall)


def time_gather(c, sd, reps, name):
    bsr, total, _ = c.scene_metrics()
    radius = 0.003 * bsr
    kw = dict(camera_pos=sd.cam_origin, mis_mode="one", pdf_mc=1.0 / math.pi / radius ** 2, clamping_value=1.0 / total, photon_radius=radius, vsl_radius=0.05 * bsr,
              vsl_inv_pi_radius2=1 / (math.pi * (0.05 * bsr) ** 2), num_light_paths=NL, num_vpl_light_paths=NL, photons_per_path=P, do_accumulate=1)
    ms = []
    for it in range(reps + 1):
        c.primary((0, 0)); c.trace_light_paths(it); c.gather_vpl(ev.frame_params(rng_seed=it, **kw)); c.synchronize()
        st = c.pass_stats(ev.PASS_GATHER_VPL)
        if it:
            ms.append(st["ms"])
    print(f"      gather over {name:22s} ms {spread(ms)}   rays {st['rays']:.3e}")
    return statistics.median(ms)


def time_quality(c, reps):
    c.profile_passes(True)
    ev_ms, wall = [], []
    for r in range(reps + 2):
        c.synchronize()
        t0 = time.perf_counter(); q = c.accel_quality(); t1 = time.perf_counter()
        if r >= 2:
            ev_ms.append(float(c.debug_accel(7))); wall.append((t1 - t0) * 1e3)
    print(f"(5) evplp_accel_quality: {q['reached_nodes']} nodes, {q['leaf_refs']} leaf references, cost {q['cost']:.3f} (root {q['root_area']:.2f}, inner {q['inner_area']:.1f}, "
          f"pairs {q['leaf_pair_area']:.1f}, triangles {q['leaf_tri_area']:.1f})")
    print(f"      device, kernel + copy of the sums ms {spread(ev_ms)}")
    print(f"      host, the call                    ms {spread(wall)}")


def chair_motions(sd, chairs, orig, small, large):
    """(name, meshes that move, vertices of every mesh) for (6)"""
    ctr = {k: 0.5 * (orig[k].min(0) + orig[k].max(0)) for k in chairs}
    rows = [sorted((k for k in chairs if ctr[k][1] < 0.0), key=lambda k: ctr[k][0]), sorted((k for k in chairs if ctr[k][1] > 3.0), key=lambda k: ctr[k][0])]

    def to_places(pairs):
        v = list(orig)
        for k, dst in pairs:
            d = ctr[dst] - ctr[k]
            v[k] = (orig[k] + np.array([d[0], d[1], 0.0], F)).astype(F)
        return [k for k, _ in pairs], v
    neigh = [p for row in rows for i in range(0, len(row) - 1, 2) for p in ((row[i], row[i + 1]), (row[i + 1], row[i]))]
    across = [p for a, b in zip(*rows) for p in ((a, b), (b, a))]
    perm = np.random.RandomState(9).permutation(len(chairs))
    shuffle = [(k, chairs[perm[i]]) for i, k in enumerate(chairs) if chairs[perm[i]] != k]
    return [("every mesh moved by a centimetre", list(range(len(sd.meshes))), small), ("every chair a metre away (seeded directions)", chairs, large),
            ("neighbouring chairs swapped", *to_places(neigh)), ("the rows of chairs swapped across the room", *to_places(across)),
            ("every chair at another chair's place (seeded)", *to_places(shuffle))]


def quality_table(sd, a, chairs, orig, small, large):
    print("(6) SAH cost (evplp_accel_quality) and config-#2 gather ms of the refitted SAH tree and of a rebuilt SAH tree of the same moved scene")
    rows = []
    for name, meshes, verts in chair_motions(sd, chairs, orig, small, large):
        print(f"    {name}: {len(meshes)} meshes moved")
        c = context(sd, a.res, ev.BVH_SAH)
        built = c.accel_quality()["cost"]
        for m in meshes:
            c.update_mesh(m, verts[m])
        c.refit_accel()
        q_refit = c.accel_quality()
        t_refit = time_gather(c, sd, a.reps, "refitted SAH")
        c.close()
        c = context(sd, a.res, ev.BVH_SAH, verts)
        q_sah = c.accel_quality()
        t_sah = time_gather(c, sd, a.reps, "rebuilt SAH")
        c.close()
        rows.append((name, built, q_refit["cost"], q_sah["cost"], q_refit["cost"] / q_sah["cost"], t_refit, t_sah, t_refit / t_sah))
    print("    motion | cost as built | cost refitted | cost rebuilt | cost ratio | gather refitted ms | gather rebuilt ms | time ratio")
    for r in rows:
        print("    %s | %.2f | %.2f | %.2f | %.3f | %.2f | %.2f | %.3f" % r)


def gather_pass(c, sd, it):
    """one config-#2 gather (time_gather's pass); returns its HIP-event ms"""
    bsr, total, _ = c.scene_metrics()
    radius = 0.003 * bsr
    kw = dict(camera_pos=sd.cam_origin, mis_mode="one", pdf_mc=1.0 / math.pi / radius ** 2, clamping_value=1.0 / total, photon_radius=radius, vsl_radius=0.05 * bsr,
              vsl_inv_pi_radius2=1 / (math.pi * (0.05 * bsr) ** 2), num_light_paths=NL, num_vpl_light_paths=NL, photons_per_path=P, do_accumulate=1)
    c.primary((0, 0)); c.trace_light_paths(it); c.gather_vpl(ev.frame_params(rng_seed=it, **kw)); c.synchronize()
    return c.pass_stats(ev.PASS_GATHER_VPL)["ms"]


def gathers_alternating(ctxs, sd, reps):
    """the gather over every context of `ctxs` {name: context}, the contexts taking turns within every repetition; {name: [ms]}"""
    ms = {n: [] for n in ctxs}
    for it in range(reps + 1):
        for n, c in ctxs.items():
            t = gather_pass(c, sd, it)
            if it:
                ms[n].append(t)
    return ms


def rotate_table(sd, a, chairs, orig, small, large):
    """(8) --rotate: tree rotations inside the refit (evplp_set_refit_rotations), on the aged tree and on fresh trees"""
    q = lambda f, xs: sorted(xs)[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]
    print("(8) tree rotations inside the refit.  Per motion: the refitted SAH tree without and with 1, 2 and 4 rotation passes, beside a rebuilt SAH tree and a")
    print("    PLOC rebuild of the same moved scene; the gathers of one motion take turns within every repetition.  A gather difference inside the p10 - p90")
    print("    spread of the refitted-only tree's gather is no difference.")
    for name, meshes, verts in chair_motions(sd, chairs, orig, small, large):
        print(f"  {name}: {len(meshes)} meshes moved")
        ctxs, notes = {}, {}
        for k in (0, 1, 2, 4):
            c = context(sd, a.res, ev.BVH_SAH)
            built = c.accel_quality()["cost"]
            c.set_refit_rotations(k)
            for m in meshes:
                c.update_mesh(m, verts[m])
            c.refit_accel()
            n = f"refitted SAH + {k} passes" if k else "refitted SAH"
            ctxs[n] = c
            notes[n] = (c.rotation_info()["last_call"], c.accel_quality()["cost"], built, c.accel_info()["stack4_entries"])
        for n, b in (("rebuilt SAH", ev.BVH_SAH), ("rebuilt PLOC", ev.BVH_PLOC_GPU)):
            ctxs[n] = context(sd, a.res, b, verts)
            notes[n] = (0, ctxs[n].accel_quality()["cost"], 0.0, ctxs[n].accel_info()["stack4_entries"])
        ms = gathers_alternating(ctxs, sd, a.reps)
        base = ms["refitted SAH"]
        floor = 0.5 * (q(0.9, base) - q(0.1, base))
        for n in ctxs:
            d = statistics.median(ms[n]) - statistics.median(base)
            verdict = "" if n == "refitted SAH" else ("   no difference (within +- %.2f ms)" % floor if abs(d) <= floor else "   %+.2f ms against the refitted-only tree" % d)
            print(f"      {n:26s} rotations {notes[n][0]:6d}   cost {notes[n][1]:9.2f}   stack4 {notes[n][3]:3d}   gather ms {spread(ms[n])}{verdict}")
        # what the refit costs with the passes on: the meshes go back and forth, every refit moves them (and rotates what it finds)
        for k in (0, 1, 2, 4):
            c = ctxs[f"refitted SAH + {k} passes" if k else "refitted SAH"]
            ev_ms, wall, rot = [], [], []
            for r in range(a.reps + 2):
                src = orig if r % 2 == 0 else verts
                for m in meshes:
                    c.update_mesh(m, src[m])
                c.synchronize()
                t0 = time.perf_counter(); c.refit_accel(); t1 = time.perf_counter()
                if r >= 2:
                    ev_ms.append(c.refit_info()["last_refit_ms"]); wall.append((t1 - t0) * 1e3); rot.append(c.rotation_info()["last_call"] if k else 0)
            print(f"      refit with {k} passes: device ms {spread(ev_ms)}   host call ms {spread(wall)}   rotations per refit, median {int(statistics.median(rot))}")
        for c in ctxs.values():
            c.close()
    print("  fresh trees of the unmoved scene: evplp_optimize_accel over a device LBVH and a PLOC tree, beside the SAH tree")
    ctxs, notes = {}, {}
    ctxs["SAH"] = context(sd, a.res, ev.BVH_SAH)
    notes["SAH"] = (0, ctxs["SAH"].accel_quality()["cost"], 0.0)
    for bn, b in (("device LBVH", GPU_BUILDER), ("PLOC", ev.BVH_PLOC_GPU)):
        for k in (0, 1, 2, 4):
            c = context(sd, a.res, b)
            c.synchronize()
            t0 = time.perf_counter(); n = c.optimize_accel(k) if k else 0; t1 = time.perf_counter()
            name = f"{bn} + {k} passes" if k else bn
            ctxs[name] = c
            notes[name] = (n, c.accel_quality()["cost"], (t1 - t0) * 1e3)
    ms = gathers_alternating(ctxs, sd, a.reps)
    for n in ctxs:
        print(f"      {n:26s} rotations {notes[n][0]:6d}   cost {notes[n][1]:9.2f}   optimize call ms {notes[n][2]:8.3f}   gather ms {spread(ms[n])}")
    for c in ctxs.values():
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--quality-only", action="store_true", help="parts (5) and (6) alone")
    ap.add_argument("--transform", action="store_true", help="part (7) alone")
    ap.add_argument("--rotate", action="store_true", help="part (8) alone: tree rotations inside the refit")
    ap.add_argument("--package-root", default=None, help="import evplp_amd from this checkout instead of the tool's own")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="evplp_refit_") as d:
        sd, _ = scenes.load_obj_scene(ev.synth_scene(d, "conf", a.tris, 1234, a.res, a.res, style="hard"))
    ntri = sum(m["idx"].shape[0] for m in sd.meshes)
    chairs = chair_meshes(sd)
    print(f"scene: {ntri} triangles in {len(sd.meshes)} meshes, {len(chairs)} chairs found; {a.reps} repetitions; median (p10 - p90)")
    orig = [m["verts"] for m in sd.meshes]
    small = [(v + np.array([0.01, 0.01, 0.0], F)).astype(F) for v in orig]
    rng = np.random.RandomState(5)
    large = list(orig)
    for k in chairs:
        ang = rng.rand() * 2 * math.pi
        large[k] = (orig[k] + np.array([math.cos(ang), math.sin(ang), 0.0], F)).astype(F)

    if a.rotate:
        rotate_table(sd, a, chairs, orig, small, large)
        return
    if a.transform:
        print(f"library: {ev.LIB_PATH}")
        one = chairs[:1] if chairs else [0]
        every = list(range(len(sd.meshes)))
        nudged = list(orig)
        nudged[one[0]] = (orig[one[0]] + np.array([0.05, 0.0, 0.0], F)).astype(F)
        eye = np.eye(3, 4, dtype=F)
        shift = lambda d: np.concatenate([np.eye(3, dtype=F), np.array(d, F).reshape(3, 1)], axis=1)
        c = context(sd, a.res, ev.BVH_SAH)
        time_moves(c, sd, one, (nudged, orig), a.reps, "one chair")
        if hasattr(c, "transform_mesh"):
            time_moves(c, sd, one, (shift((0.05, 0.0, 0.0)), eye), a.reps, "one chair")
        time_moves(c, sd, every, (small, orig), a.reps, "every mesh")
        if hasattr(c, "transform_mesh"):
            time_moves(c, sd, every, (shift((0.01, 0.01, 0.0)), eye), a.reps, "every mesh")
            time_moves(c, sd, one, (nudged, orig), a.reps, "one chair, after the transforms,")
        c.close()
        return
    if a.quality_only:
        c = context(sd, a.res, ev.BVH_SAH)
        time_quality(c, a.reps)
        c.close()
        quality_table(sd, a, chairs, orig, small, large)
        return
    c = context(sd, a.res, ev.BVH_SAH)
    one = chairs[:1] if chairs else [0]
    nudged = list(orig)
    nudged[one[0]] = (orig[one[0]] + np.array([0.05, 0.0, 0.0], F)).astype(F)
    time_refits(c, sd, one, (nudged, orig), a.reps, "(a) one chair")
    every = list(range(len(sd.meshes)))
    refit_ms, refit_wall = time_refits(c, sd, every, (small, orig), a.reps, "(b) every mesh, small translation")
    time_quality(c, a.reps)
    sah_wall = time_builds(c, a.reps, "SAH (host)")
    c.close()
    g = context(sd, a.res, GPU_BUILDER)
    gpu_wall = time_builds(g, a.reps, "device LBVH")
    g.close()
    print(f"    refit (b) / SAH rebuild, wall: {refit_wall / sah_wall:.4f}   refit (b) / device LBVH rebuild, wall: {refit_wall / gpu_wall:.4f}")

    for tag, verts in (("(3) small motion (b)", small), ("(4) every chair a metre away", large)):
        print(f"{tag}: the config-#2 gather over three trees of the same moved scene")
        c = context(sd, a.res, ev.BVH_SAH)
        for m in (every if verts is small else chairs):
            c.update_mesh(m, verts[m])
        c.refit_accel()
        t_refit = time_gather(c, sd, a.reps, "refitted SAH")
        c.close()
        c = context(sd, a.res, ev.BVH_SAH, verts)
        t_sah = time_gather(c, sd, a.reps, "rebuilt SAH")
        c.close()
        c = context(sd, a.res, GPU_BUILDER, verts)
        t_gpu = time_gather(c, sd, a.reps, "rebuilt device LBVH")
        c.close()
        print(f"      refitted / rebuilt SAH: {t_refit / t_sah:.3f}   refitted SAH / rebuilt device LBVH: {t_refit / t_gpu:.3f}   rebuilt device LBVH / rebuilt SAH: {t_gpu / t_sah:.3f}")
    quality_table(sd, a, chairs, orig, small, large)


if __name__ == "__main__":
    main()
