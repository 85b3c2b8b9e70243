"""evplp_transform_mesh + evplp_refit_accel: a mesh moved by a 3 x 4 matrix on the device, from its rest pose.  The yardstick of every case
is a context that was handed the same positions through evplp_update_mesh -- the positions being evplp.transform_points of the rest pose,
the function the library itself moves the mesh with -- and, where stated, a fresh build of the moved scene.  Every comparison is of bytes:
every plane, the records, the ray and pair counters, the scene's figures."""
import json
import math
import os
import shutil

import numpy as np
import pytest

from test_gpu_refit import (BUILDERS, JITTER, NPATHS, H, P, W, box_meshes, fresh, group_frame_params, lit, motion_light, moved_room, render, room,  # noqa: F401
                            tiny_context, tiny_render, tiny_scene)

pytestmark = pytest.mark.gpu
F = np.float32
IDENTITY = np.eye(3, 4, dtype=F).reshape(12)


# ---- matrices (row-major 3 x 4), and the motions they make: {mesh: matrix} -> {mesh: positions}
def translation(d):
    m = np.eye(3, 4, dtype=F); m[:, 3] = d
    return m.reshape(12)


def rotation_z(room, meshes, degrees):
    """about the vertical through the centre of the meshes' bounding box"""
    allv = np.concatenate([room.meshes[m]["verts"] for m in meshes]).astype(np.float64)
    cx, cy = 0.5 * (allv.min(0) + allv.max(0))[:2]
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return np.array([c, -s, 0, cx - c * cx + s * cy, s, c, 0, cy - s * cx - c * cy, 0, 0, 1, 0], F)


def scale(k):
    return np.array([k[0], 0, 0, 0, 0, k[1], 0, 0, 0, 0, k[2], 0], F)


def matrices_a(room):
    ms = {m: translation((0.35, -0.2, 0.0)) for m in box_meshes(0)}
    ms.update({m: rotation_z(room, box_meshes(2), 25.0) for m in box_meshes(2)})
    ms.update({m: scale((1.1, 0.9, 1.4)) for m in box_meshes(4)})
    return ms


def positions(evplp, room, matrices):
    return {m: evplp.transform_points(mat, room.meshes[m]["verts"]) for m, mat in matrices.items()}


def transform(c, matrices):
    for m, mat in matrices.items():
        c.transform_mesh(m, mat)


def update(c, motion):
    for m, v in motion.items():
        c.update_mesh(m, v)


def context(evplp, room, builder="sah"):
    c = evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True)
    room.upload(c)
    return c


def frame(evplp, c):
    r = render(evplp, c)
    r["metrics"] = c.scene_metrics()
    return r


def same(got, want, what):
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == v, f"{what}: {k} differs"


def by_update(evplp, room, motion, builder="sah", accel=False):
    """the yardstick: the same positions through evplp_update_mesh, one refit"""
    with context(evplp, room, builder) as c:
        update(c, motion)
        c.refit_accel()
        r = frame(evplp, c)
        if accel:
            r.update({f"accel {w}": c.debug_accel(w).tobytes() for w in range(5)})
    return r


def fresh_build(evplp, room, motion):
    return fresh(evplp, moved_room(room, motion))


# ---- 1
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_gaps_and_a_ragged_end(evplp, room, builder):
    ms = matrices_a(room)
    assert sorted(ms) == list(range(6, 12)) + list(range(18, 24)) + list(range(30, 36))
    moved = sum(len(room.meshes[m]["idx"].reshape(-1, 3)) for m in ms)
    assert moved % 256 != 0 and (3 * moved) % 256 != 0 and 3 * moved > 256, "a ragged last workgroup, and more than one"
    mo = positions(evplp, room, ms)
    want = by_update(evplp, room, mo, builder, accel=True)
    assert lit(want) and want["pos"] != fresh(evplp, room)["pos"], "the motion is not visible"
    with context(evplp, room, builder) as c:
        transform(c, ms)
        c.refit_accel()
        got = frame(evplp, c)
        got.update({f"accel {w}": c.debug_accel(w).tobytes() for w in range(5)})
        assert c.refit_info()["refits"] == 1
    same(got, want, f"{builder}: three boxes by three matrices against the update path")
    fb = fresh_build(evplp, room, mo)
    same({k: got[k] for k in fb}, fb, f"{builder}: against a fresh build of the moved room")


# ---- 2
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_transform_and_upload_in_one_refit(evplp, room, builder):
    ms = {m: translation((0.35, -0.2, 0.0)) for m in box_meshes(0)}
    up = {m: room.meshes[m]["verts"] + np.array([-0.3, 0.25, 0.0], F) for m in box_meshes(5)}
    mo = dict(positions(evplp, room, ms)); mo.update(up)
    want = by_update(evplp, room, mo, builder)
    with context(evplp, room, builder) as c:
        transform(c, ms)
        update(c, up)
        c.refit_accel()
        same(frame(evplp, c), want, f"{builder}: box 0 by matrix, box 5 by upload")
    same(want, fresh_build(evplp, room, mo), "the yardstick against a fresh build")


# ---- 3
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_transforms_do_not_compose_and_do_not_drift(evplp, room, builder):
    a = {m: rotation_z(room, box_meshes(2), 25.0) for m in box_meshes(2)}
    b = {m: rotation_z(room, box_meshes(2), -40.0) for m in box_meshes(2)}
    ident = {m: IDENTITY for m in box_meshes(2)}
    want_b = by_update(evplp, room, positions(evplp, room, b), builder)
    want_i = by_update(evplp, room, positions(evplp, room, ident), builder)
    with context(evplp, room, builder) as c:
        transform(c, b); c.refit_accel()
        same(frame(evplp, c), want_b, "a context that only ever saw B")
    with context(evplp, room, builder) as c:
        transform(c, a); c.refit_accel()
        assert frame(evplp, c)["pos"] != want_b["pos"]
        transform(c, b); c.refit_accel()
        same(frame(evplp, c), want_b, f"{builder}: A then B is B of the rest pose")
        transform(c, a); transform(c, b); c.refit_accel()                     # (the second call replaces the first before a refit too)
        same(frame(evplp, c), want_b, f"{builder}: A, B, one refit")
        transform(c, ident); c.refit_accel()
        same(frame(evplp, c), want_i, f"{builder}: the identity gives the rest pose back")
        assert c.refit_info()["refits"] == 4


# ---- 4
def test_update_mesh_sets_a_new_rest_pose(evplp, room):
    meshes = box_meshes(2)
    a = {m: translation((0.2, 0.1, 0.0)) for m in meshes}
    v1 = {m: room.meshes[m]["verts"] * np.array([1, 1, 1.3], F) for m in meshes}
    mm = {m: rotation_z(room, meshes, 30.0) for m in meshes}
    final = {m: evplp.transform_points(mm[m], v1[m]) for m in meshes}
    want = by_update(evplp, room, final)
    assert want["pos"] != by_update(evplp, room, positions(evplp, room, mm))["pos"], "the new rest pose must show"
    with context(evplp, room) as c:
        transform(c, a); c.refit_accel()
        update(c, v1); c.refit_accel()
        transform(c, mm); c.refit_accel()
        same(frame(evplp, c), want, "transform, update, transform: three refits")
    with context(evplp, room) as c:
        transform(c, a); c.refit_accel()
        update(c, v1); transform(c, mm); c.refit_accel()
        same(frame(evplp, c), want, "update then transform in front of one refit")
    with context(evplp, room) as c:
        update(c, v1); transform(c, mm); c.refit_accel()                      # (a mesh that never had a matrix: the rest pose comes from the host)
        same(frame(evplp, c), want, "update then transform, the mesh's first matrix")
        transform(c, a); update(c, v1); c.refit_accel()                       # the update forgets the matrix
        same(frame(evplp, c), by_update(evplp, room, v1), "transform then update: the upload wins")


# ---- 5
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_the_light_moves(evplp, room, builder):
    lm = room.light_mesh
    v = room.meshes[lm]["verts"]
    cx = float(F(0.5) * (v[:, 0].min() + v[:, 0].max()))
    ms = {lm: np.array([1.2, 0, 0, cx * (1 - 1.2), 0, 1, 0, 0, 0, 0, 1, -0.4], F), 1: translation((0.5, 0, 0))}
    mo = positions(evplp, room, ms)
    ref = motion_light(room)
    assert all(np.abs(mo[m] - ref[m]).max() < 1e-5 for m in ms), "the motion of motion_light, as matrices"
    want = fresh_build(evplp, room, mo)
    orig = fresh(evplp, room)
    assert want["metrics"][0] != orig["metrics"][0] and want["metrics"][2] != orig["metrics"][2]     # radius and light area
    assert want["records"] != orig["records"]
    with context(evplp, room, builder) as c:
        transform(c, ms)
        c.refit_accel()
        assert c.scene_metrics() == want["metrics"]
        same(frame(evplp, c), want, f"{builder}: light and wall by matrix against a fresh build")
    same(by_update(evplp, room, mo, builder), want, "the update path")


# ---- 6
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_one_triangle_and_degenerate_meshes(evplp, builder):
    down = translation((0, -0.25, 0))
    for ntri in (1, 9):
        light, lidx, floor = tiny_scene(ntri)
        with tiny_context(evplp, "sah", light, lidx, evplp.transform_points(down, floor))[0] as c:
            want = tiny_render(evplp, c)
        c, fm = tiny_context(evplp, builder, light, lidx, floor)
        with c:
            orig = tiny_render(evplp, c)
            c.transform_mesh(fm, down)
            c.refit_accel()
            assert tiny_render(evplp, c) == want and want[0] != orig[0], ntri
    # a zero scale switches the mesh off in place: a fresh build drops all of it
    light, lidx, floor = tiny_scene(9)
    zero = np.zeros(12, F)
    with tiny_context(evplp, "sah", light, lidx, evplp.transform_points(zero, floor))[0] as c:
        want_off = tiny_render(evplp, c), c.scene_metrics()
    with tiny_context(evplp, "sah", light, lidx, evplp.transform_points(IDENTITY, floor))[0] as c:
        want_on = tiny_render(evplp, c), c.scene_metrics()
    c, fm = tiny_context(evplp, builder, light, lidx, floor)
    with c:
        c.transform_mesh(fm, zero)
        c.refit_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_off
        c.transform_mesh(fm, IDENTITY)                                        # the matrix that brings it back: every triangle still has its leaf
        c.refit_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_on and want_on[0][0] != want_off[0][0]
        # ... but a tree BUILT while the mesh was off dropped its triangles: a matrix that gives them an area is refused by the refit
        c.transform_mesh(fm, zero)
        c.build_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_off
        c.transform_mesh(fm, IDENTITY)
        with pytest.raises(evplp.EvplpError) as e:
            c.refit_accel()
        assert e.value.status == evplp.ERR_INVALID and "had no area when the tree was built and has one now" in str(e.value) and "evplp_build_accel" in str(e.value)
        with pytest.raises(evplp.EvplpError):                                 # still dirty
            c.primary((0.0, 0.0), clear_light=True)
        c.build_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_on


# ---- 7
def test_rebuilds_keep_the_rest_pose(evplp, room):
    meshes = box_meshes(2)
    a = {m: rotation_z(room, meshes, 25.0) for m in meshes}
    b = {m: rotation_z(room, meshes, -40.0) for m in meshes}
    d = {m: translation((0.0, 0.3, 0.1)) for m in meshes}
    want = {k: by_update(evplp, room, positions(evplp, room, ms)) for k, ms in (("a", a), ("b", b), ("d", d))}
    with context(evplp, room) as c:
        c.set_refit_policy(1e-3, BUILDERS["gpu"])                             # any refit costs more than a thousandth of the built tree: it rebuilds
        transform(c, a); c.refit_accel()
        assert c.accel_quality()["last_action"] == 2 and c.accel_quality()["policy_rebuilds"] == 1
        same(frame(evplp, c), want["a"], "A, policy rebuild")
        transform(c, b); c.refit_accel()
        assert c.accel_quality()["policy_rebuilds"] == 2
        same(frame(evplp, c), want["b"], "B after a policy rebuild starts from the rest pose")
        c.set_refit_policy(0.0)
        transform(c, d); c.refit_accel()                                      # a plain refit of the rebuilt tree: the kernel, from the host's rest pose
        assert c.accel_quality()["policy_rebuilds"] == 2
        same(frame(evplp, c), want["d"], "D by the kernel after the rebuilds")
    with context(evplp, room) as c:
        transform(c, a); c.refit_accel()
        transform(c, b); c.build_accel()                                      # the full rebuild on a dirty context
        same(frame(evplp, c), want["b"], "build_accel on a context dirty by transform")
        transform(c, d); c.refit_accel()
        same(frame(evplp, c), want["d"], "D after build_accel starts from the rest pose")
        assert c.refit_info()["refits"] == 2


# ---- 8
def test_refusals_and_the_dirty_state(evplp, room):
    L = evplp.lib()
    m0 = box_meshes(0)[0]
    good = translation((0.35, -0.2, 0.0))
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        mat = c.add_material((0.5, 0.5, 0.5), (0, 0, 0), 0.0)
        c.add_mesh(room.meshes[0]["verts"], room.meshes[0]["idx"], mat)
        with pytest.raises(evplp.EvplpError) as e:                            # no accel built
            c.transform_mesh(0, good)
        assert e.value.status == evplp.ERR_INVALID and "evplp_build_accel" in str(e.value)
    ms = {m: good for m in box_meshes(0)}
    want = by_update(evplp, room, positions(evplp, room, ms))
    with context(evplp, room) as c:
        before = frame(evplp, c)
        nan, inf, over = good.copy(), good.copy(), good.copy()
        nan[5] = np.nan; inf[3] = np.inf; over[0] = 3e38                      # 3e38 x: the product overflows, every entry is finite
        assert np.isfinite(over).all() and np.abs(room.meshes[m0]["verts"][:, 0]).max() > 2
        for args in ((-1, good), (len(room.meshes), good), (m0, nan), (m0, inf), (m0, over)):
            with pytest.raises(evplp.EvplpError) as e:
                c.transform_mesh(*args)
            assert e.value.status == evplp.ERR_INVALID, args
            same(frame(evplp, c), before, "nothing was marked by a refused transform: the context renders, and renders the same")
        assert "not finite under the matrix" in str(e.value)
        assert L.evplp_transform_mesh(c._h, m0, None) == evplp.ERR_INVALID
        c.refit_accel()
        assert c.refit_info()["refits"] == 0
        transform(c, ms)
        cam = c.camera()
        fp = evplp.frame_params(camera_pos=list(cam.origin), num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
        for call in (lambda: c.primary(JITTER, clear_light=True), lambda: c.trace_light_paths(7), lambda: c.gather_vpl(fp), lambda: c.gather_lvc(fp),
                     lambda: c.splat_photons(fp, clear=True), lambda: c.path_trace(list(cam.origin), 5, 3)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value) and "evplp_build_accel" in str(e.value)
        with pytest.raises(evplp.EvplpError):                                 # a refusal on a dirty context leaves it dirty, and as it was
            c.transform_mesh(m0, over)
        c.refit_accel()
        same(frame(evplp, c), want, "after the refusals")
        assert c.refit_info()["refits"] == 1


# ---- 9
def test_a_context_that_never_transforms_allocates_nothing_new(evplp):
    """Device memory in use around the first refit of a large mesh: after evplp_update_mesh alone it grows by the refit's own arrays (28 B per
    node + 36 B per triangle + 4 B per light triangle; include/evplp.h), within the allocator's granularity; the first evplp_transform_mesh
    then adds the rest pose, 36 B per triangle -- which shows that the figure would see it."""
    import torch
    n = 600
    g = np.linspace(-5, 5, n + 1, dtype=F)
    x, y = np.meshgrid(g, g)
    verts = np.stack([x.ravel(), y.ravel(), (0.05 * np.sin(3 * x) * np.cos(2 * y)).ravel()], axis=1).astype(F)
    i = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    idx = np.concatenate([np.stack([i, i + 1, i + n + 2], 1), np.stack([i, i + n + 2, i + n + 1], 1)]).astype(np.int32)
    ntri = len(idx)
    assert ntri == 2 * n * n
    light = np.array([[-1, -1, 4], [1, -1, 4], [1, 1, 4], [-1, 1, 4]], F)
    with evplp.Context(32, 32, 16, 16, 4, bvh_builder=BUILDERS["gpu"]) as c:
        mat = c.add_material((0.6, 0.6, 0.6), (0.0, 0.0, 0.0), 1.0)
        lm = c.add_mesh(light, np.array([[0, 2, 1], [0, 3, 2]], np.int32), mat)
        fm = c.add_mesh(verts, idx, mat)
        c.set_arealight(lm, (10.0, 10.0, 10.0, 0.0))
        c.set_camera((0.0, -8.0, 3.0), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.9, 1.0)
        c.build_accel()
        c.primary((0.0, 0.0), clear_light=True); c.synchronize()

        def in_use():
            torch.cuda.synchronize()
            free, total = torch.cuda.mem_get_info(0)
            return total - free
        m0 = in_use()
        c.update_mesh(fm, verts + np.array([0, 0, 0.1], F))
        c.refit_accel(); c.synchronize()
        m1 = in_use()
        c.update_mesh(fm, verts)
        c.refit_accel(); c.synchronize()
        m2 = in_use()
        c.transform_mesh(fm, translation((0, 0, 0.1)))
        m3 = in_use()
        c.refit_accel(); c.synchronize()
        m4 = in_use()
        nodes = c.accel_info()["nodes"]
    todays = 28 * nodes + 36 * ntri + 4 * 2
    rest = 36 * ntri
    slack = 8 << 20                                                           # (three device allocations, each rounded up by the allocator)
    assert rest > 2 * slack
    print(f"refit by upload: +{m1 - m0} B (today's arrays: {todays} B), second: +{m2 - m1} B; first transform: +{m3 - m2} B (rest pose: {rest} B); its refit: +{m4 - m3} B")
    assert m1 - m0 <= todays + slack, "a refit after update_mesh alone allocates more than the refit's own arrays"
    assert m2 - m1 <= 0, "the second refit allocates"
    assert rest <= m3 - m2 <= rest + slack, "the rest pose is made by the first transform, and by it alone"
    assert m4 - m3 <= 0


# ---- 10
def group_frame(evplp, g, room, total, n_iter=1):
    g.clear_accumulators()
    js = [JITTER, (-0.003, 0.002)]
    for i in range(n_iter):
        if n_iter > 1:
            g.select_rank(i)
        fp = group_frame_params(evplp, room, total, 7 + i)
        g.primary(js[i], 1) if n_iter == 1 else g.primary(js[i])
        g.trace_light_paths(7 + i); g.gather(fp, 0); g.splat_photons(fp)
    s = 1.0 / n_iter
    return g.resolve(s, s, 1.0).tobytes()


def test_groups(evplp, room):
    a, b = matrices_a(room), {m: rotation_z(room, box_meshes(2), -40.0) for m in box_meshes(2)}
    want = {}
    with context(evplp, room) as c:
        for k, ms in (("a", a), ("b", b)):
            update(c, positions(evplp, room, ms) if k == "a" else {**positions(evplp, room, {m: IDENTITY for m in a}), **positions(evplp, room, b)})
            c.refit_accel()
            _, total, _ = c.scene_metrics()
            fp = group_frame_params(evplp, room, total, 7)
            c.clear_accumulators()
            c.primary(JITTER, clear_light=True); c.trace_light_paths(7); c.gather_vpl(fp); c.splat_photons(fp)
            want[k] = c.resolve(1.0, 1.0, 1.0)[:H].tobytes(), total
    assert np.frombuffer(want["a"][0], F).max() > 0 and want["a"][0] != want["b"][0]
    reset = {m: IDENTITY for m in a}
    for n in (2, 4):
        with evplp.Group(W, H, NPATHS, NPATHS, P, n, devices=[0] * n, deterministic=True) as g:
            for r in range(n):
                room.upload(g.rank(r))
            with pytest.raises(evplp.EvplpError) as e:                        # refused on the caller's thread: the group stays usable
                g.transform_mesh(len(room.meshes), IDENTITY)
            assert e.value.status == evplp.ERR_INVALID
            for m, mat in a.items():
                g.transform_mesh(m, mat)
            with pytest.raises(evplp.EvplpError) as e:
                g.primary(JITTER, 1)
            assert e.value.status == evplp.ERR_INVALID and "evplp_group_refit_accel" in str(e.value)
            g.refit_accel()
            assert all(g.rank(r).refit_info()["refits"] == 1 for r in range(n))
            assert group_frame(evplp, g, room, want["a"][1]) == want["a"][0], f"{n} ranks, strips round robin"
            # the strips dealt by cost
            g.calibrate(True)
            group_frame(evplp, g, room, want["a"][1])
            g.rebalance()
            for m, mat in {**reset, **b}.items():
                g.transform_mesh(m, mat)
            g.refit_accel()
            assert group_frame(evplp, g, room, want["b"][1]) == want["b"][0], f"{n} ranks, strips dealt {g.block_owners().tolist()}"
    # the iteration partition: against the same group moved by upload
    frames = []
    for by_matrix in (False, True):
        with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True, partition="iterations") as g:
            for r in range(2):
                room.upload(g.rank(r))
            for m, mat in a.items():
                g.transform_mesh(m, mat) if by_matrix else g.update_mesh(m, evplp.transform_points(mat, room.meshes[m]["verts"]))
            g.refit_accel()
            frames.append(group_frame(evplp, g, room, want["a"][1], n_iter=2))
    assert frames[0] == frames[1] and np.frombuffer(frames[0], np.uint8).any()


# ---- 11: the "animation" block of the technique JSON against plain renders of scenes whose OBJ files hold the moved vertices
def _obj_lines(path):
    return open(path).read().split("\n")


def _moved_obj(evplp, src, dst, matrix, group=None):
    """src with its `v` lines under the matrix (group: only those between the group-th `usemtl` and the next; None: all), written with %.9g"""
    lines = _obj_lines(src)
    g, rows = -1, []
    for i, ln in enumerate(lines):
        if ln.startswith("usemtl"):
            g += 1
        if ln.startswith("v ") and (group is None or g == group):
            rows.append(i)
    pts = np.array([[float(t) for t in lines[i].split()[1:4]] for i in rows], np.float64).astype(F)
    assert len(rows) > 0 and all(("%.9g" % float(v)) == t for i, p in zip(rows, pts) for v, t in zip(p, lines[i].split()[1:4])), "the file holds fp32 numbers as %.9g"
    out = evplp.transform_points(matrix, pts)
    for i, p in zip(rows, out):
        lines[i] = "v %.9g %.9g %.9g" % (float(p[0]), float(p[1]), float(p[2]))
    open(dst, "w").write("\n".join(lines))
    return len(rows)


def _box_obj(path, lo, hi, material):
    c = [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    s = ["mtllib room.mtl", f"usemtl {material}"]
    for p in c:
        s += ["v %.9g %.9g %.9g" % tuple(float(F(v)) for v in p), "vt 0 0"]
    for a, b, d, e in quads:
        s += [f"f {a + 1}/{a + 1} {b + 1}/{b + 1} {d + 1}/{d + 1}", f"f {a + 1}/{a + 1} {d + 1}/{d + 1} {e + 1}/{e + 1}"]
    open(path, "w").write("\n".join(s) + "\n")


def _anim_matrices(f):
    c, s = math.cos(math.radians(20.0 * (f + 1))), math.sin(math.radians(20.0 * (f + 1)))
    cx, cy = 12.0, -2.0
    box = [c, -s, 0, cx - c * cx + s * cy + 0.3 * f, s, c, 0, cy - s * cx - c * cy - 0.2 * f, 0, 0, 1.0 + 0.25 * f, 0]
    floor = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.15 * (f + 1)]
    return [float(F(v)) for v in box], [float(F(v)) for v in floor]


PT = {"rngOffset": 3, "numMaxIteration": 2, "timeLimitMs": 1e9, "frameMode": "accumulate", "outputFilename": "pt.pfm", "statFilename": "pt.json", "useJitter": True,
      "useStat": True, "numSamplePerPixel": 1, "numMaxBounces": 3}
OUTPUTS = {"photonfam": ("room_combined.pfm", "room_weightedvpl.pfm", "room_weightedpm.pfm"), "pt": ("pt.pfm",)}


def _scene_dir(evplp, tmp_path, name, technique, move=None):
    """a directory with the room, one more object (a box) and the technique block; move = (box matrix, floor matrix) rewrites the OBJ files"""
    d = tmp_path / name
    d.mkdir()
    src = tmp_path / "src"
    if not src.exists():
        src.mkdir()
        evplp.synth_scene(str(src), "room", 600, 1, W, H)
        _box_obj(str(src / "extra.obj"), (11.0, -3.0, 0.0), (13.0, -1.0, 1.5), "obj3")
    for f in ("room.mtl", "room_lights.obj"):
        shutil.copy(src / f, d / f)
    if move is None:
        shutil.copy(src / "room.obj", d / "room.obj"); shutil.copy(src / "extra.obj", d / "extra.obj")
    else:
        assert _moved_obj(evplp, str(src / "extra.obj"), str(d / "extra.obj"), move[0]) == 8
        assert _moved_obj(evplp, str(src / "room.obj"), str(d / "room.obj"), move[1], group=0) > 8
    root = json.load(open(src / "room.json"))
    root["scene"] = ["room.obj", "extra.obj"]
    fam = root.pop("photonfam")
    fam.update({"numMaxIteration": 2, "deterministic": True, "radiusPercentage": 0.02, "run": {"photonSplat": True}, "rngOffset": 3})
    root[technique] = fam if technique == "photonfam" else dict(PT)
    (d / "room.json").write_text(json.dumps(root))
    return d


@pytest.mark.parametrize("technique", ["photonfam", "pt"])
def test_animation_block(evplp, tmp_path, technique):
    frames = 3
    mats = [_anim_matrices(f) for f in range(frames)]
    want = []
    for f in range(frames):
        d = _scene_dir(evplp, tmp_path, f"ref{f}", technique, move=mats[f])
        evplp.render_json(str(d / "room.json"))
        names = sorted(p.name for p in d.iterdir())
        assert not [n for n in names if "_f0" in n], f"without the block the file names are the old ones: {names}"
        want.append({n: (d / n).read_bytes() for n in OUTPUTS[technique]})
    assert want[0] != want[1] and want[1] != want[2], "the motion is not visible"
    block = {"animation": {"frames": frames, "tracks": [{"object": 1, "matrices": [m[0] for m in mats]}, {"mesh": 0, "matrices": [m[1] for m in mats]}]}}
    runs = [("one", block)]
    if technique == "photonfam":
        runs.append(("two", dict(block, device={"gpus": 2, "virtual": True})))
        runs.append(("policy", {"animation": dict(block["animation"], refitPolicy={"maxCostRatio": 1e-3, "rebuildBuilder": "gpu"})}))
    for name, overrides in runs:
        d = _scene_dir(evplp, tmp_path, f"anim_{technique}_{name}", technique)
        evplp.render_json(str(d / "room.json"), json.dumps(overrides))
        for f in range(frames):
            for n in OUTPUTS[technique]:
                stem, ext = os.path.splitext(n)
                p = d / f"{stem}_f{f:04d}{ext}"
                assert p.exists(), (name, sorted(q.name for q in d.iterdir()))
                assert p.read_bytes() == want[f][n], f"{technique}, {name}: frame {f}, {n} differs from a plain render of the moved scene"
            stat = json.load(open(d / (("room_stat" if technique == "photonfam" else "pt") + f"_f{f:04d}.json")))
            assert stat["frame"] == f and stat["numIterations"] == 2 and stat["refitLastAction"] == (2 if name == "policy" else 0), stat
            assert (name == "policy") == ("refitCostRatio" in stat), stat
        assert not [n for n in OUTPUTS[technique] if (d / n).exists()], "every file the block writes carries its frame"
