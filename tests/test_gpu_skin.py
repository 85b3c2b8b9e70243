"""evplp_set_mesh_skin + evplp_pose_mesh + evplp_refit_accel: a mesh posed by bone matrices on the device, from its rest pose.  The yardstick
of every case is test_gpu_transform.py's: a context that was handed the same positions through evplp_update_mesh -- the positions being
evplp.skin_points of the rest pose, the function the library itself poses the mesh with -- and, where stated, a fresh build of the posed
scene.  Every comparison is of bytes: every plane, the records, the ray and pair counters, the scene's figures.

A "bend" is two or three bones along a box's height with weights that are a function of the rest position alone, so the six face meshes of
a box stay joined."""
import json
import shutil

import numpy as np
import pytest

from test_gpu_refit import BUILDERS, JITTER, NPATHS, H, P, W, box_meshes, fresh, group_frame_params, lit, room, tiny_context, tiny_render, tiny_scene  # noqa: F401
from test_gpu_transform import (IDENTITY, OUTPUTS, _box_obj, _obj_lines, by_update, context, frame, fresh_build, group_frame, rotation_z, same, transform, translation,
                                update)

pytestmark = pytest.mark.gpu
F = np.float32


# ---- skins and palettes: {mesh: (bone indices (n, 4), weights (n, 4))}, {mesh: palette (nbones, 12)} -> {mesh: positions}
def height(room, meshes):
    z = np.concatenate([room.meshes[m]["verts"][:, 2] for m in meshes])
    return F(z.min()), F(z.max())


def bend_skin(room, meshes, nbones, bones=None):
    """weights along the height of the meshes' bounding box: bone 0 at the bottom, the last at the top, linear between neighbours"""
    z0, z1 = height(room, meshes)
    bones = list(range(nbones)) if bones is None else bones
    out = {}
    for m in meshes:
        t = ((room.meshes[m]["verts"][:, 2] - z0) / (z1 - z0)).astype(F) * F(nbones - 1)
        k = np.minimum(t.astype(np.int32), max(nbones - 2, 0))
        f = (t - k.astype(F)).astype(F)
        idx = np.zeros((len(t), 4), np.int32); w = np.zeros((len(t), 4), F)
        if nbones == 1:
            idx[:, 0] = bones[0]; w[:, 0] = 1
        else:
            idx[:, 0] = np.asarray(bones, np.int32)[k]; idx[:, 1] = np.asarray(bones, np.int32)[k + 1]
            w[:, 0] = F(1) - f; w[:, 1] = f
        out[m] = (idx, w)
    return out


def bend_palette(room, meshes, degrees, shift=(0.0, 0.0, 0.0)):
    """bone k: the rotation by degrees[k] about the vertical through the meshes' centre, then k / (n - 1) of the shift"""
    n = len(degrees)
    pal = np.stack([rotation_z(room, meshes, d) for d in degrees]).astype(F)
    for k in range(n):
        pal[k, 3::4] += np.asarray(shift, F) * F(k / max(n - 1, 1))
    return {m: pal for m in meshes}


def positions(evplp, room, skins, palettes):
    return {m: evplp.skin_points(pal, skins[m][0], skins[m][1], room.meshes[m]["verts"]) for m, pal in palettes.items()}


def set_skins(c, skins, nbones):
    for m, (idx, w) in skins.items():
        c.set_mesh_skin(m, nbones[m] if isinstance(nbones, dict) else nbones, idx, w)


def pose(c, palettes):
    for m, pal in palettes.items():
        c.pose_mesh(m, pal)


def with_accel(evplp, c):
    r = frame(evplp, c)
    r.update({f"accel {w}": c.debug_accel(w).tobytes() for w in range(5)})
    return r


def bends_a(room):
    """boxes 0, 2 and 4 by three different bends: two bones, three bones, two bones with a shift"""
    skins, pals, nb = {}, {}, {}
    for b, n, deg, shift in ((0, 2, (0.0, 35.0), (0.0, 0.0, 0.0)), (2, 3, (0.0, 20.0, -30.0), (0.2, -0.1, 0.0)), (4, 2, (10.0, -25.0), (0.15, 0.2, 0.3))):
        skins.update(bend_skin(room, box_meshes(b), n)); pals.update(bend_palette(room, box_meshes(b), deg, shift)); nb.update({m: n for m in box_meshes(b)})
    return skins, pals, nb


# ---- 1
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_gaps_and_a_ragged_end(evplp, room, builder):
    skins, pals, nb = bends_a(room)
    assert sorted(pals) == list(range(6, 12)) + list(range(18, 24)) + list(range(30, 36))
    corners = 3 * sum(len(room.meshes[m]["idx"].reshape(-1, 3)) for m in pals)
    assert corners > 256 and corners % 256 != 0, "a ragged last workgroup, and more than one"
    mo = positions(evplp, room, skins, pals)
    assert all(np.abs(mo[m] - room.meshes[m]["verts"]).max() > 0.05 for m in (box_meshes(0)[0], box_meshes(2)[0], box_meshes(4)[0]))
    want = by_update(evplp, room, mo, builder, accel=True)
    assert lit(want) and want["pos"] != fresh(evplp, room)["pos"], "the motion is not visible"
    with context(evplp, room, builder) as c:
        set_skins(c, skins, nb)
        same(frame(evplp, c), fresh(evplp, room, builder), "a skin moves nothing and marks nothing dirty")
        pose(c, pals)
        c.refit_accel()
        got = with_accel(evplp, c)
        assert c.refit_info()["refits"] == 1
    same(got, want, f"{builder}: three boxes by three bends against the update path")
    fb = fresh_build(evplp, room, mo)
    same({k: got[k] for k in fb}, fb, f"{builder}: against a fresh build of the posed room")


# ---- 2
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_three_kinds_in_one_refit(evplp, room, builder):
    skins = bend_skin(room, box_meshes(0), 2); pals = bend_palette(room, box_meshes(0), (0.0, 35.0))
    ms = {m: rotation_z(room, box_meshes(2), 25.0) for m in box_meshes(2)}
    up = {m: room.meshes[m]["verts"] + np.array([-0.3, 0.25, 0.0], F) for m in box_meshes(5)}
    mo = dict(positions(evplp, room, skins, pals))
    mo.update({m: evplp.transform_points(mat, room.meshes[m]["verts"]) for m, mat in ms.items()}); mo.update(up)
    want = by_update(evplp, room, mo, builder)
    with context(evplp, room, builder) as c:
        set_skins(c, skins, 2)
        update(c, up); pose(c, pals); transform(c, ms)
        c.refit_accel()
        same(frame(evplp, c), want, f"{builder}: box 0 by bones, box 2 by matrix, box 5 by upload")
        assert c.refit_info()["refits"] == 1
    same(want, fresh_build(evplp, room, mo), "the yardstick against a fresh build")


# ---- 3
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_poses_do_not_compose_and_do_not_drift(evplp, room, builder):
    meshes = box_meshes(2)
    skins = bend_skin(room, meshes, 3)
    a, b = bend_palette(room, meshes, (0.0, 20.0, -30.0), (0.2, -0.1, 0.0)), bend_palette(room, meshes, (5.0, -40.0, 15.0), (-0.1, 0.2, 0.1))
    rest = {m: np.tile(IDENTITY, (3, 1)) for m in meshes}
    mat = {m: rotation_z(room, meshes, 25.0) for m in meshes}
    want_b = by_update(evplp, room, positions(evplp, room, skins, b), builder)
    want_r = by_update(evplp, room, positions(evplp, room, skins, rest), builder)
    want_m = by_update(evplp, room, {m: evplp.transform_points(mat[m], room.meshes[m]["verts"]) for m in meshes}, builder)
    with context(evplp, room, builder) as c:
        set_skins(c, skins, 3)
        pose(c, b); c.refit_accel()
        same(frame(evplp, c), want_b, "a context that only ever saw B")
    with context(evplp, room, builder) as c:
        set_skins(c, skins, 3)
        pose(c, a); c.refit_accel()
        assert frame(evplp, c)["pos"] != want_b["pos"]
        pose(c, b); c.refit_accel()
        same(frame(evplp, c), want_b, f"{builder}: A then B is B of the rest pose")
        pose(c, a); pose(c, b); c.refit_accel()                                # (the second call replaces the first before a refit too)
        same(frame(evplp, c), want_b, f"{builder}: A, B, one refit")
        for i in range(50):
            pose(c, a if i % 2 == 0 else b); c.refit_accel()
        pose(c, rest); c.refit_accel()
        same(frame(evplp, c), want_r, f"{builder}: fifty alternating poses, then the rest palette")
        pose(c, a); transform(c, mat); c.refit_accel()
        same(frame(evplp, c), want_m, f"{builder}: pose then transform: the matrix wins")
        transform(c, mat); pose(c, b); c.refit_accel()
        same(frame(evplp, c), want_b, f"{builder}: transform then pose: the pose wins")
        transform(c, mat); c.refit_accel(); pose(c, b); c.refit_accel()
        same(frame(evplp, c), want_b, f"{builder}: the same over two refits: the pose is of the rest pose, not of the moved mesh")
        assert c.refit_info()["refits"] == 58


def test_update_mesh_sets_a_new_rest_pose_and_keeps_the_skin(evplp, room):
    meshes = box_meshes(2)
    skins = bend_skin(room, meshes, 2)
    a, b = bend_palette(room, meshes, (0.0, 35.0)), bend_palette(room, meshes, (10.0, -25.0), (0.1, 0.0, 0.0))
    v1 = {m: room.meshes[m]["verts"] * np.array([1, 1, 1.3], F) for m in meshes}
    final = {m: evplp.skin_points(b[m], skins[m][0], skins[m][1], v1[m]) for m in meshes}
    want = by_update(evplp, room, final)
    assert want["pos"] != by_update(evplp, room, positions(evplp, room, skins, b))["pos"], "the new rest pose must show"
    with context(evplp, room) as c:
        set_skins(c, skins, 2)
        pose(c, a); c.refit_accel()
        update(c, v1); c.refit_accel()
        same(frame(evplp, c), by_update(evplp, room, v1), "the update forgets the pose")
        pose(c, b); c.refit_accel()
        same(frame(evplp, c), want, "pose, update, pose: three refits")
    with context(evplp, room) as c:
        set_skins(c, skins, 2)
        update(c, v1); pose(c, b); c.refit_accel()                             # (a mesh that never had a pose: the rest pose comes from the host)
        same(frame(evplp, c), want, "update then pose in front of one refit")


@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_a_new_skin_between_pose_and_refit(evplp, room, builder):
    """evplp_set_mesh_skin on a mesh whose pose no refit has taken: the posed positions stay and go up by upload, which overwrites the
    attributes the device's rest pose was still to be taken from -- it must come from the host's rest pose, or every later pose skins the
    posed positions.  On clean meshes that never had a matrix or a pose (the rest pose is not on the device yet), and on meshes that had."""
    meshes = box_meshes(2)
    s2, s3 = bend_skin(room, meshes, 2), bend_skin(room, meshes, 3)
    a = bend_palette(room, meshes, (0.0, 35.0), (0.1, 0.0, 0.0))
    b = bend_palette(room, meshes, (5.0, -40.0, 15.0), (-0.1, 0.2, 0.1))
    d = bend_palette(room, meshes, (0.0, 20.0, -30.0), (0.2, -0.1, 0.0))
    want_a = by_update(evplp, room, positions(evplp, room, s2, a), builder)
    want_b = by_update(evplp, room, positions(evplp, room, s3, b), builder)
    want_d = by_update(evplp, room, positions(evplp, room, s3, d), builder)
    assert want_a["pos"] != want_b["pos"] and want_b["pos"] != want_d["pos"]
    for warm in (False, True):
        with context(evplp, room, builder) as c:
            set_skins(c, s2, 2)
            if warm:                                                           # the device holds the rest pose before the sequence starts
                pose(c, a); c.refit_accel()
            pose(c, a)
            set_skins(c, s3, 3)                                                # the new skin, in front of the refit: the mesh goes up by upload
            for m in meshes:
                assert c.mesh_vertices(m, 0).tobytes() == positions(evplp, room, s2, a)[m].tobytes() and c.mesh_vertices(m, 1).tobytes() == room.meshes[m]["verts"].tobytes()
            with pytest.raises(evplp.EvplpError):                              # still dirty
                c.primary(JITTER, clear_light=True)
            c.refit_accel()
            same(frame(evplp, c), want_a, f"{builder}, warm {warm}: the pose under the old skin stays, by upload")
            pose(c, b); c.refit_accel()
            same(frame(evplp, c), want_b, f"{builder}, warm {warm}: the next pose is of the REST pose under the new skin")
            pose(c, d); c.refit_accel()
            same(frame(evplp, c), want_d, f"{builder}, warm {warm}: and the one after it")


# ---- 4
def test_palette_edges(evplp, room):
    meshes = box_meshes(3)
    rng = np.random.default_rng(5)
    cases = {}
    # one bone
    cases["one bone"] = (1, bend_skin(room, meshes, 1), {m: rotation_z(room, meshes, 33.0).reshape(1, 12) for m in meshes})
    # 1024 bones, the bend between bone 0 and bone 1023; every entry between them is a different finite matrix nobody may read
    pal = rng.uniform(-3, 3, (1024, 12)).astype(F)
    two = bend_palette(room, meshes, (0.0, 35.0), (0.1, 0.1, 0.0))[meshes[0]]
    pal[0], pal[1023] = two[0], two[1]
    cases["1024 bones"] = (1024, bend_skin(room, meshes, 2, bones=[0, 1023]), {m: pal for m in meshes})
    # four distinct bones on every vertex: two pairs of bones, each pair shares the bend's weight in halves
    sk = {}
    for m, (idx, w) in bend_skin(room, meshes, 2).items():
        i4 = np.tile(np.array([0, 1, 2, 3], np.int32), (len(idx), 1))
        w4 = np.stack([w[:, 0] * F(0.5), w[:, 1] * F(0.5), w[:, 0] * F(0.5), w[:, 1] * F(0.5)], 1).astype(F)
        sk[m] = (i4, w4)
    four = np.stack([rotation_z(room, meshes, d) for d in (0.0, 30.0, 6.0, 40.0)]).astype(F)
    cases["four distinct bones"] = (4, sk, {m: four for m in meshes})
    assert all(len(set(r)) == 4 for r in sk[meshes[0]][0].tolist()) and (sk[meshes[0]][1] > 0).all(1).any()
    seen = set()
    for name, (nb, skins, pals) in cases.items():
        mo = positions(evplp, room, skins, pals)
        want = by_update(evplp, room, mo)
        assert want["pos"] not in seen, name
        seen.add(want["pos"])
        with context(evplp, room) as c:
            set_skins(c, skins, nb)
            pose(c, pals); c.refit_accel()
            same(frame(evplp, c), want, name)
    one = cases["one bone"]
    assert np.array_equal(positions(evplp, room, one[1], one[2])[meshes[0]], evplp.transform_points(one[2][meshes[0]][0], room.meshes[meshes[0]]["verts"]))


# ---- 5
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_the_light_posed(evplp, room, builder):
    lm = room.light_mesh
    v = room.meshes[lm]["verts"]
    x0, x1 = F(v[:, 0].min()), F(v[:, 0].max())
    t = ((v[:, 0] - x0) / (x1 - x0)).astype(F)
    idx = np.tile(np.array([0, 1, 0, 0], np.int32), (len(v), 1))
    w = np.stack([F(1) - t, t, np.zeros_like(t), np.zeros_like(t)], 1).astype(F)
    skins = {lm: (idx, w)}
    pals = {lm: np.stack([translation((-0.3, 0.0, -0.4)), translation((0.4, 0.0, -0.2))]).astype(F)}    # stretched along x, lowered and tilted
    mo = positions(evplp, room, skins, pals)
    want = fresh_build(evplp, room, mo)
    orig = fresh(evplp, room)
    assert want["metrics"][2] != orig["metrics"][2] and want["records"] != orig["records"]               # the light's area, the light-traced records
    with context(evplp, room, builder) as c:
        set_skins(c, skins, 2)
        pose(c, pals)
        c.refit_accel()
        assert c.scene_metrics() == want["metrics"]
        same(frame(evplp, c), want, f"{builder}: the light by bones against a fresh build")
    same(by_update(evplp, room, mo, builder), want, "the update path")


# ---- 6
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_degenerate_meshes(evplp, builder):
    light, lidx, floor = tiny_scene(9)
    t = ((floor[:, 0] + F(1)) / F(2)).astype(F)
    idx = np.tile(np.array([0, 1, 1, 0], np.int32), (len(floor), 1))
    w = np.stack([F(1) - t, t * F(0.5), t * F(0.5), np.zeros_like(t)], 1).astype(F)
    zero = np.zeros((2, 12), F)
    down = np.stack([translation((0, -0.25, 0)), translation((0, -0.5, 0))]).astype(F)
    off_v, on_v = evplp.skin_points(zero, idx, w, floor), evplp.skin_points(down, idx, w, floor)
    assert not off_v.any()
    with tiny_context(evplp, "sah", light, lidx, off_v)[0] as c:
        want_off = tiny_render(evplp, c), c.scene_metrics()
    with tiny_context(evplp, "sah", light, lidx, on_v)[0] as c:
        want_on = tiny_render(evplp, c), c.scene_metrics()
    c, fm = tiny_context(evplp, builder, light, lidx, floor)
    with c:
        c.set_mesh_skin(fm, 2, idx, w)
        c.pose_mesh(fm, zero)                                                  # a palette of zero matrices switches the mesh off in place
        c.refit_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_off
        c.pose_mesh(fm, down)                                                  # the next pose brings it back: every triangle still has its leaf
        c.refit_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_on and want_on[0][0] != want_off[0][0]
        # ... but a tree BUILT while the mesh was off dropped its triangles: a pose that gives them an area is refused by the refit
        c.pose_mesh(fm, zero)
        c.build_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_off
        c.pose_mesh(fm, down)
        with pytest.raises(evplp.EvplpError) as e:
            c.refit_accel()
        assert e.value.status == evplp.ERR_INVALID and "had no area when the tree was built and has one now" in str(e.value) and "evplp_build_accel" in str(e.value)
        with pytest.raises(evplp.EvplpError):                                 # still dirty
            c.primary((0.0, 0.0), clear_light=True)
        c.build_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_on


# ---- 7
def test_refusals_and_the_dirty_state(evplp, room):
    L = evplp.lib()
    meshes = box_meshes(0)
    m0 = meshes[0]
    skins = bend_skin(room, meshes, 2); pals = bend_palette(room, meshes, (0.0, 35.0))
    idx, w = skins[m0]
    n = len(idx)
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        mat = c.add_material((0.5, 0.5, 0.5), (0, 0, 0), 0.0)
        c.add_mesh(room.meshes[m0]["verts"], room.meshes[m0]["idx"], mat)
        for call in (lambda: c.set_mesh_skin(0, 2, idx, w), lambda: c.pose_mesh(0, pals[m0])):
            with pytest.raises(evplp.EvplpError) as e:                        # no accel built
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_build_accel" in str(e.value)
    want = by_update(evplp, room, positions(evplp, room, skins, pals))

    def edit(a, at, v):
        a = a.copy(); a[at] = v
        return a
    with context(evplp, room) as c:
        before = frame(evplp, c)

        def refused(call, what, needle=None):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID, what
            assert needle is None or needle in str(e.value), (what, str(e.value))
        with pytest.raises(evplp.EvplpError):
            c.pose_mesh(m0, pals[m0])                                          # the mesh has no skin
        zw = tuple(np.argwhere(w == 0)[0])
        bad_sum = w.copy(); bad_sum[2] = bad_sum[2] * F(1.002)
        skin_cases = {"mesh < 0": (-1, 2, idx, w), "mesh = count": (len(room.meshes), 2, idx, w), "a vertex too few": (m0, 2, idx[:-1], w[:-1]),
                      "a vertex too many": (m0, 2, np.concatenate([idx, idx[:1]]), np.concatenate([w, w[:1]])), "nbones < 0": (m0, -1, idx, w), "nbones = 1025": (m0, 1025, idx, w),
                      "index = nbones": (m0, 2, edit(idx, (1, 0), 2), w), "index < 0": (m0, 2, edit(idx, (1, 0), -1), w), "index out of range under a zero weight": (m0, 2, edit(idx, zw, 7), w),
                      "weight nan": (m0, 2, idx, edit(w, (1, 0), np.nan)), "weight inf": (m0, 2, idx, edit(w, (1, 0), np.inf)),
                      "weight < 0": (m0, 2, idx, edit(edit(w, (1, 2), -0.25), (1, 3), 0.25)), "weights add up to 1.002": (m0, 2, idx, bad_sum)}
        for what, args in skin_cases.items():
            refused(lambda: c.set_mesh_skin(*args), what)
            same(frame(evplp, c), before, f"{what}: nothing was changed by a refused skin: the context renders, and renders the same")
        for null_args in ((None, w.ctypes.data), (idx.ctypes.data, None)):
            assert L.evplp_set_mesh_skin(c._h, m0, 2, null_args[0], null_args[1], n) == evplp.ERR_INVALID
            same(frame(evplp, c), before, "a null pointer: nothing was changed by a refused skin")
        refused(lambda: c.pose_mesh(m0, pals[m0]), "still no skin", "has no skin")
        set_skins(c, skins, 2)
        same(frame(evplp, c), before, "a skin marks nothing dirty")
        good = pals[m0]
        over = edit(good, (1, 0), 3e38)                                        # 3e38 x: the product overflows, every entry is finite
        assert np.isfinite(over).all() and np.abs(room.meshes[m0]["verts"][:, 0]).max() > 2
        pose_cases = {"mesh < 0": (-1, good), "mesh = count": (len(room.meshes), good), "a mesh without a skin": (box_meshes(1)[0], good), "a bone too few": (m0, good[:1]),
                      "a bone too many": (m0, np.concatenate([good, good[:1]])), "matrix nan": (m0, edit(good, (0, 5), np.nan)), "matrix inf": (m0, edit(good, (1, 3), np.inf)),
                      "a posed coordinate that is not finite": (m0, over)}
        for what, args in pose_cases.items():
            refused(lambda: c.pose_mesh(*args), what)
            same(frame(evplp, c), before, f"{what}: nothing was marked by a refused pose")
        refused(lambda: c.pose_mesh(m0, over), "over", "not finite under the palette")
        assert L.evplp_pose_mesh(c._h, m0, None, 2) == evplp.ERR_INVALID
        same(frame(evplp, c), before, "a null palette: nothing was marked by a refused pose")
        c.refit_accel()
        assert c.refit_info()["refits"] == 0
        pose(c, pals)
        cam = c.camera()
        fp = evplp.frame_params(camera_pos=list(cam.origin), num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
        for call in (lambda: c.primary(JITTER, clear_light=True), lambda: c.trace_light_paths(7), lambda: c.gather_vpl(fp), lambda: c.gather_lvc(fp),
                     lambda: c.splat_photons(fp, clear=True), lambda: c.path_trace(list(cam.origin), 5, 3)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value) and "evplp_build_accel" in str(e.value)
        refused(lambda: c.pose_mesh(m0, over), "a refusal on a dirty context leaves it dirty, and as it was")
        c.refit_accel()
        same(frame(evplp, c), want, "after the refusals")
        assert c.refit_info()["refits"] == 1
        # the skin removed: the pose is refused again, the posed positions stay
        for m in meshes:
            c.set_mesh_skin(m, 0)
        refused(lambda: c.pose_mesh(m0, good), "the skin was removed", "has no skin")
        same(frame(evplp, c), want, "removing a skin moves nothing")


# ---- 8
def test_rebuilds_keep_the_skin(evplp, room):
    meshes = box_meshes(2)
    skins = bend_skin(room, meshes, 3)
    a = bend_palette(room, meshes, (0.0, 20.0, -30.0), (0.2, -0.1, 0.0))
    b = bend_palette(room, meshes, (5.0, -40.0, 15.0), (-0.1, 0.2, 0.1))
    d = bend_palette(room, meshes, (0.0, 10.0, 45.0))
    want = {k: by_update(evplp, room, positions(evplp, room, skins, p)) for k, p in (("a", a), ("b", b), ("d", d))}
    with context(evplp, room) as c:
        set_skins(c, skins, 3)
        c.set_refit_policy(1e-3, BUILDERS["gpu"])                             # any refit costs more than a thousandth of the built tree: it rebuilds
        pose(c, a); c.refit_accel()
        assert c.accel_quality()["last_action"] == 2 and c.accel_quality()["policy_rebuilds"] == 1
        same(frame(evplp, c), want["a"], "A, policy rebuild")
        pose(c, b); c.refit_accel()
        assert c.accel_quality()["policy_rebuilds"] == 2
        same(frame(evplp, c), want["b"], "B after a policy rebuild starts from the rest pose, under the kept skin")
        c.set_refit_policy(0.0)
        pose(c, d); c.refit_accel()                                           # a plain refit of the rebuilt tree: the kernel, the skin sent again
        assert c.accel_quality()["policy_rebuilds"] == 2
        same(frame(evplp, c), want["d"], "D by the kernel after the rebuilds")
    with context(evplp, room) as c:
        set_skins(c, skins, 3)
        pose(c, a); c.refit_accel()
        pose(c, b); c.build_accel()                                           # the full rebuild on a context dirty by pose
        same(frame(evplp, c), want["b"], "build_accel on a context dirty by pose")
        pose(c, d); c.refit_accel()
        same(frame(evplp, c), want["d"], "D after build_accel: the skin survived it")
        assert c.refit_info()["refits"] == 2


# ---- 9
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_rotations_on(evplp, room, builder):
    skins, pals, nb = bends_a(room)
    mo = positions(evplp, room, skins, pals)
    with context(evplp, room, builder) as c:
        c.set_refit_rotations(1)
        update(c, mo); c.refit_accel()
        want = with_accel(evplp, c)
        want_rot = c.rotation_info()
    with context(evplp, room, builder) as c:
        c.set_refit_rotations(1)
        set_skins(c, skins, nb)
        pose(c, pals); c.refit_accel()
        same(with_accel(evplp, c), want, f"{builder}: a posed refit with rotations against the same setting over the update path")
        assert c.rotation_info() == want_rot


# ---- 10
def test_groups(evplp, room):
    skins, pals, nb = bends_a(room)
    mo = positions(evplp, room, skins, pals)
    with context(evplp, room) as c:
        update(c, mo); c.refit_accel()
        _, total, _ = c.scene_metrics()
        fp = group_frame_params(evplp, room, total, 7)
        c.clear_accumulators()
        c.primary(JITTER, clear_light=True); c.trace_light_paths(7); c.gather_vpl(fp); c.splat_photons(fp)
        want = c.resolve(1.0, 1.0, 1.0)[:H].tobytes()
    assert np.frombuffer(want, F).max() > 0
    m0 = box_meshes(0)[0]
    with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True) as g:
        for r in range(2):
            room.upload(g.rank(r))
        for call in (lambda: g.set_mesh_skin(len(room.meshes), 2, *skins[m0]), lambda: g.set_mesh_skin(m0, 2, skins[m0][0][:-1], skins[m0][1][:-1]),
                     lambda: g.pose_mesh(m0, pals[m0])):                       # (the last: no skin yet) refused on the caller's thread: the group stays usable
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID
        set_skins(g, skins, nb)
        with pytest.raises(evplp.EvplpError) as e:
            g.pose_mesh(m0, pals[m0][:1])
        assert e.value.status == evplp.ERR_INVALID
        pose(g, pals)
        with pytest.raises(evplp.EvplpError) as e:
            g.primary(JITTER, 1)
        assert e.value.status == evplp.ERR_INVALID and "evplp_group_refit_accel" in str(e.value)
        g.refit_accel()
        assert all(g.rank(r).refit_info()["refits"] == 1 for r in range(2))
        assert group_frame(evplp, g, room, total) == want, "2 ranks, strips"
    frames = []
    for by_bones in (False, True):
        with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True, partition="iterations") as g:
            for r in range(2):
                room.upload(g.rank(r))
            if by_bones:
                set_skins(g, skins, nb); pose(g, pals)
            else:
                update(g, mo)
            g.refit_accel()
            frames.append(group_frame(evplp, g, room, total, n_iter=2))
    assert frames[0] == frames[1] and np.frombuffer(frames[0], np.uint8).any()


# ---- 11: a "poses" track of the technique JSON against plain renders of scenes whose OBJ file holds the posed vertices
BOX_LO, BOX_HI = (11.0, -3.0, 0.0), (13.0, -1.0, 1.5)


def _bend_of(p):
    """the skin of the extra box as a function of the position: two bones along its height"""
    t = (p[:, 2] / F(BOX_HI[2])).astype(F)
    idx = np.tile(np.array([0, 1, 0, 0], np.int32), (len(p), 1))
    return idx, np.stack([F(1) - t, t, np.zeros_like(t), np.zeros_like(t)], 1).astype(F)


def _palette(f):
    m = np.eye(3, 4, dtype=F); m[0, 1] = 0.2 * (f + 1); m[:, 3] = (0.3 * (f + 1), -0.4, 0.25 * f)
    return np.stack([IDENTITY, m.reshape(12)]).astype(F)


def _scene_dir(evplp, tmp_path, name, palette=None):
    d = tmp_path / name
    d.mkdir()
    src = tmp_path / "src"
    if not src.exists():
        src.mkdir()
        evplp.synth_scene(str(src), "room", 600, 1, W, H)
        _box_obj(str(src / "extra.obj"), BOX_LO, BOX_HI, "obj3")
    for f in ("room.mtl", "room_lights.obj", "room.obj", "extra.obj"):
        shutil.copy(src / f, d / f)
    if palette is not None:
        lines = _obj_lines(str(src / "extra.obj"))
        rows = [i for i, ln in enumerate(lines) if ln.startswith("v ")]
        pts = np.array([[float(t) for t in lines[i].split()[1:4]] for i in rows], np.float64).astype(F)
        out = evplp.skin_points(palette, *_bend_of(pts), pts)
        for i, p in zip(rows, out):
            lines[i] = "v %.9g %.9g %.9g" % (float(p[0]), float(p[1]), float(p[2]))
        open(d / "extra.obj", "w").write("\n".join(lines))
    root = json.load(open(src / "room.json"))
    root["scene"] = ["room.obj", "extra.obj"]
    fam = root.pop("photonfam")
    fam.update({"numMaxIteration": 2, "deterministic": True, "radiusPercentage": 0.02, "run": {"photonSplat": True}, "rngOffset": 3, "timeLimitMs": 1e9})
    root["photonfam"] = fam
    (d / "room.json").write_text(json.dumps(root))
    return d


def test_poses_track(evplp, tmp_path):
    frames = 2
    want = []
    for f in range(frames):
        d = _scene_dir(evplp, tmp_path, f"ref{f}", _palette(f))
        evplp.render_json(str(d / "room.json"))
        want.append({n: (d / n).read_bytes() for n in OUTPUTS["photonfam"]})
    assert want[0] != want[1], "the motion is not visible"
    d = _scene_dir(evplp, tmp_path, "anim")
    # vertex v is the loader's numbering: the queries return it
    with evplp.Context(W, H, NPATHS, NPATHS, P) as c:
        c.load_scene_json(str(d / "room.json"))
        n = c.mesh_count()
        box = [m for m in range(n) if c.mesh_info(m)["nverts"] == 8 and (c.mesh_vertices(m) >= np.array(BOX_LO, F)).all() and (c.mesh_vertices(m) <= np.array(BOX_HI, F)).all()]
        assert len(box) == 1 and c.mesh_info(box[0])["ntris"] == 12
        verts = c.mesh_vertices(box[0])
    idx, w = _bend_of(verts)
    track = {"mesh": box[0], "skin": {"bones": 2, "indices": idx.tolist(), "weights": [[float(x) for x in r] for r in w]},
             "poses": [[[float(x) for x in m] for m in _palette(f)] for f in range(frames)]}
    evplp.render_json(str(d / "room.json"), json.dumps({"animation": {"frames": frames, "tracks": [track]}}))
    for f in range(frames):
        for name in OUTPUTS["photonfam"]:
            stem, ext = name.rsplit(".", 1)
            p = d / f"{stem}_f{f:04d}.{ext}"
            assert p.exists(), sorted(q.name for q in d.iterdir())
            assert p.read_bytes() == want[f][name], f"frame {f}, {name} differs from a plain render of the posed scene"
    # a wrong vertex count is the C call's refusal, said by the track's name
    short = dict(track, skin=dict(track["skin"], indices=track["skin"]["indices"][:-1], weights=track["skin"]["weights"][:-1]))
    d2 = _scene_dir(evplp, tmp_path, "short")
    with pytest.raises(evplp.EvplpError) as e:
        evplp.render_json(str(d2 / "room.json"), json.dumps({"animation": {"frames": frames, "tracks": [short]}}))
    assert "animation.tracks[0].skin" in str(e.value) and "8 vertices, not 7" in str(e.value), str(e.value)
    assert not [q.name for q in d2.iterdir() if q.suffix == ".pfm"]


# ---- 12
def test_temporal(evplp):
    import test_gpu_temporal as tt
    box = tt.make_box()
    meshes = tt.BOX_MESHES
    z = np.concatenate([box.meshes[m]["verts"][:, 2] for m in meshes])
    z0, z1 = F(z.min()), F(z.max())
    skins = {}
    for m in meshes:
        t = ((box.meshes[m]["verts"][:, 2] - z0) / (z1 - z0)).astype(F)
        skins[m] = (np.tile(np.array([0, 1, 0, 0], np.int32), (len(t), 1)), np.stack([F(1) - t, t, np.zeros_like(t), np.zeros_like(t)], 1).astype(F))
    pal = np.stack([IDENTITY, tt.box_matrix(box, 0.08, (-0.2, 0.15, 0.0)).reshape(12)]).astype(F)
    out = []
    for by_bones in (False, True):
        with evplp.Context(tt.W, tt.H, 1, 1, 1) as c:
            box.upload(c); c.noise_track(True); c.temporal_enable(True)
            if by_bones:
                set_skins(c, skins, 2)
            tt.render(evplp, c, box.cam_origin, 0)
            imgs = [c.denoise_temporal(1.0 / tt.ITERS)[0].tobytes()]
            for m in meshes:
                c.pose_mesh(m, pal) if by_bones else c.update_mesh(m, evplp.skin_points(pal, skins[m][0], skins[m][1], box.meshes[m]["verts"]))
            c.refit_accel()
            tt.render(evplp, c, box.cam_origin, 1)
            img, info = c.denoise_temporal(1.0 / tt.ITERS)
            imgs.append(img.tobytes())
            out.append((imgs, info, tuple(c.temporal_download(k).tobytes() for k in range(3))))
    assert out[1][1]["reprojected"] > 0 and out[1][1]["frames_since_reset"] == 2
    assert out[0][0][0] != out[0][0][1], "the motion is not visible"
    assert out[1][0] == out[0][0] and out[1][1] == out[0][1] and out[1][2] == out[0][2], "two frames of a posed box against the same frames through evplp_update_mesh"


# ---- 13
def test_queries(evplp, room):
    m0 = box_meshes(2)[1]
    skins = bend_skin(room, [m0], 2); pals = bend_palette(room, [m0], (0.0, 35.0), (0.1, 0.0, 0.2))
    L = evplp.lib()
    with context(evplp, room) as c:
        assert c.mesh_count() == len(room.meshes)
        for m, sd in enumerate(room.meshes):
            info = c.mesh_info(m)
            assert info["nverts"] == len(sd["verts"]) and info["ntris"] == len(np.asarray(sd["idx"]).reshape(-1, 3)), m
            for which in (0, 1):
                assert c.mesh_vertices(m, which).tobytes() == np.ascontiguousarray(sd["verts"], F).tobytes(), (m, which)
        assert len({c.mesh_info(m)["material"] for m in range(c.mesh_count())}) > 1
        set_skins(c, skins, 2); pose(c, pals)
        posed = positions(evplp, room, skins, pals)[m0]
        assert c.mesh_vertices(m0, 0).tobytes() == posed.tobytes() and c.mesh_vertices(m0, 1).tobytes() == room.meshes[m0]["verts"].tobytes()
        c.refit_accel()
        assert c.mesh_vertices(m0, 0).tobytes() == posed.tobytes() and c.mesh_vertices(m0, 1).tobytes() == room.meshes[m0]["verts"].tobytes()
        c.update_mesh(m0, posed); c.refit_accel()                              # a new rest pose
        assert c.mesh_vertices(m0, 1).tobytes() == posed.tobytes()
        out = np.zeros((64, 3), F)
        n = c.mesh_info(m0)["nverts"]
        for args in ((-1, 0, out.ctypes.data, 64), (c.mesh_count(), 0, out.ctypes.data, 64), (m0, 2, out.ctypes.data, 64), (m0, 0, None, 64), (m0, 0, out.ctypes.data, n - 1)):
            assert L.evplp_mesh_vertices(c._h, *args) == evplp.ERR_INVALID, args
        assert not out.any() and L.evplp_mesh_info(c._h, c.mesh_count(), None, None, None) == evplp.ERR_INVALID
        assert L.evplp_mesh_info(c._h, m0, None, None, None) == evplp.OK
