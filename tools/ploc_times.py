"""What the device PLOC builder (EVPLP_BVH_PLOC_GPU) costs to build and buys the gather, beside the host SAH builder and the device LBVH.  One
process, the furnished stand-in (evplp_synth_scene, style "hard", 331 k triangles), `reps` repetitions each, median with p10 - p90.

  (1) per builder -- SAH, device LBVH, PLOC at radius 4, 8, 16, 32 (EVPLP_PLOC_RADIUS, read when the context is created):
      accel_info()["build_ms"] and the wall time of evplp_build_accel; PLOC's iteration count (evplp_ploc_tree, the host twin: the same tree);
      nodes, leaf blocks, depth; the evplp_accel_quality cost; the config-#2 gather (tools/refit_times.py's pass) in ms per pass.
  (2) the moved scene "every chair at another chair's place" (the one motion of DESIGN section 6b outside the noise): the gather over the
      refitted SAH tree against the gather over a PLOC rebuild (and a SAH and a device-LBVH rebuild) of the moved scene, and the refit's
      time against the PLOC build's.

usage: python tools/ploc_times.py [--reps N] [--tris N] [--res N]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refit_times as rt  # noqa: E402  (the scene, the gather pass and the chair motions are its)
from refit_times import ev, scenes  # noqa: E402

RADII = (4, 8, 16, 32)


def builders():
    yield "SAH (host)", ev.BVH_SAH, None
    yield "device LBVH", ev.BVH_LBVH_GPU, None
    for r in RADII:
        yield f"PLOC r = {r}", ev.BVH_PLOC_GPU, r


def context(sd, res, builder, radius, verts=None):
    if radius is None:
        os.environ.pop("EVPLP_PLOC_RADIUS", None)
    else:
        os.environ["EVPLP_PLOC_RADIUS"] = str(radius)
    try:
        return rt.context(sd, res, builder, verts)
    finally:
        os.environ.pop("EVPLP_PLOC_RADIUS", None)


def time_builds(c, reps):
    ms, wall = [], []
    for _ in range(reps):
        c.synchronize()
        t0 = time.perf_counter(); c.build_accel(); c.synchronize(); wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(c.accel_info()["build_ms"])
    return ms, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--tris", type=int, default=331000)
    ap.add_argument("--res", type=int, default=1024)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="evplp_ploc_") as d:
        sd, _ = scenes.load_obj_scene(ev.synth_scene(d, "conf", a.tris, 1234, a.res, a.res, style="hard"))
    soup = sd.triangle_soup()[0]
    chairs = rt.chair_meshes(sd)
    print(f"scene: {soup.shape[0]} triangles in {len(sd.meshes)} meshes, {len(chairs)} chairs found; {a.reps} repetitions; median (p10 - p90)")

    print("(1) builders on the scene as loaded")
    rows = []
    for name, builder, radius in builders():
        c = context(sd, a.res, builder, radius)
        ms, wall = time_builds(c, a.reps)
        info, q = c.accel_info(), c.accel_quality()
        assert info["builder"] == {ev.BVH_SAH: "sah", ev.BVH_LBVH_GPU: "gpu", ev.BVH_PLOC_GPU: "ploc"}[builder], info
        its = ev.ploc_tree(soup, radius)[2] if radius is not None else 0
        print(f"    {name}: build_ms {rt.spread(ms)}   wall ms {rt.spread(wall)}   {info}")
        g = rt.time_gather(c, sd, a.reps, name)
        c.close()
        rows.append((name, statistics.median(ms), statistics.median(wall), its, info["nodes"], info["leaves"], info["depth"], q["cost"], g))
    print("    builder | build_ms | wall ms | iterations | nodes | leaf blocks | depth | SAH cost | gather ms per pass")
    for r in rows:
        print("    %s | %.2f | %.2f | %d | %d | %d | %d | %.2f | %.2f" % r)

    print("(2) every chair at another chair's place (seeded): the refitted SAH tree against rebuilds of the moved scene")
    orig = [m["verts"] for m in sd.meshes]
    name, meshes, verts = rt.chair_motions(sd, chairs, orig, orig, orig)[-1]
    c = context(sd, a.res, ev.BVH_SAH, None)
    refit_ms = []
    for r in range(a.reps + 2):                                               # there and back: every refit really moves the chairs
        c.synchronize()
        t0 = time.perf_counter()
        for m in meshes:
            c.update_mesh(m, (verts if r % 2 == 0 else orig)[m])
        c.refit_accel(); c.synchronize()
        if r >= 2:
            refit_ms.append((time.perf_counter() - t0) * 1e3)
    for m in meshes:
        c.update_mesh(m, verts[m])
    c.refit_accel()
    q_refit = c.accel_quality()["cost"]
    g_refit = rt.time_gather(c, sd, a.reps, "refitted SAH")
    c.close()
    print(f"    update + refit, wall ms {rt.spread(refit_ms)}   cost {q_refit:.2f}")
    print("    tree of the moved scene | SAH cost | wall ms of what made it | gather ms per pass | gather / refitted SAH's")
    print("    refitted SAH | %.2f | %.2f | %.2f | 1.000" % (q_refit, statistics.median(refit_ms), g_refit))
    for bname, builder, radius in (("SAH (host)", ev.BVH_SAH, None), ("device LBVH", ev.BVH_LBVH_GPU, None), ("PLOC r = 16", ev.BVH_PLOC_GPU, 16)):
        c = context(sd, a.res, builder, radius, verts)
        _, wall = time_builds(c, max(a.reps // 4, 3))
        q = c.accel_quality()["cost"]
        g = rt.time_gather(c, sd, a.reps, "rebuilt " + bname)
        c.close()
        print("    rebuilt %s | %.2f | %.2f | %.2f | %.3f" % (bname, q, statistics.median(wall), g, g / g_refit))


if __name__ == "__main__":
    main()
