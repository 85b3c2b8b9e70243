"""evplp_set_mesh_morph + evplp_morph_mesh + evplp_refit_accel: a mesh blended from its rest pose and morph targets on the device, alone or
under the matrix or the pose in force.  The yardstick of every case is test_gpu_transform.py's: a context that was handed the same positions
through evplp_update_mesh -- the positions being the numpy fp32 restatement of morph_point (test_morph_host.restate_morph) of the rest pose,
then evplp.transform_points / evplp.skin_points where a matrix or a pose acts on that base -- and, where stated, a fresh build of the moved
scene.  Every comparison is of bytes: every plane, the records, the ray and pair counters, the scene's figures, the device's tree.

A target is a function of the rest position alone, so the six face meshes of a box stay joined."""
import copy
import json
import shutil

import numpy as np
import pytest

from test_gpu_refit import BUILDERS, JITTER, NPATHS, H, P, W, box_meshes, fresh, group_frame_params, lit, room, tiny_context, tiny_render, tiny_scene  # noqa: F401
from test_gpu_skin import bend_palette, bend_skin, set_skins
from test_gpu_transform import IDENTITY, OUTPUTS, _box_obj, _obj_lines, by_update, context, frame, fresh_build, group_frame, rotation_z, same, transform, translation, update
from test_morph_host import restate_morph

pytestmark = pytest.mark.gpu
F = np.float32


# ---- targets and weights: {mesh: deltas (T, n, 3)}, {mesh: weights (T,)} -> {mesh: positions}
def targets_of(room, meshes, T, amp=0.04):
    """target k: a swelling about the centre of the meshes' bounding box, growing with the height, plus a small shift along axis k % 3"""
    allv = np.concatenate([room.meshes[m]["verts"] for m in meshes])
    lo, hi = allv.min(0), allv.max(0)
    ctr = F(0.5) * (lo + hi)
    span = np.maximum(hi - lo, F(1e-3))
    out = {}
    for m in meshes:
        v = room.meshes[m]["verts"]
        t = ((v[:, 2] - lo[2]) / span[2]).astype(F)
        d = np.empty((T,) + v.shape, F)
        for k in range(T):
            s = F(amp * (1 + k % 4) * (-1 if k % 2 else 1))
            d[k] = (v - ctr) * s * (F(0.25) + t)[:, None]
            d[k][:, k % 3] += F(0.02 * (1 + k % 7))
        out[m] = d
    return out


def weights_of(seed, T):
    """weights of 0.3 .. 1.5 -- beyond 1 is extrapolation --, every third one negative, and a zero among three or more"""
    w = np.random.default_rng(seed).uniform(0.3, 1.5, T).astype(F)
    w[2::3] *= F(-1)
    if T >= 3:
        w[1] = 0.0                                                             # a zero weight is evaluated like any other
    return w


def bases(room, targets, weights, rest=None):
    return {m: restate_morph(room.meshes[m]["verts"] if rest is None else rest[m], targets[m], weights[m]) for m in weights}


def set_targets(c, targets):
    for m, d in targets.items():
        c.set_mesh_morph(m, d)


def morph(c, weights):
    for m, w in weights.items():
        c.morph_mesh(m, w)


def unmorph(c, meshes):
    for m in meshes:
        c.morph_mesh(m, None)


def with_accel(evplp, c):
    r = frame(evplp, c)
    r.update({f"accel {w}": c.debug_accel(w).tobytes() for w in range(5)})
    return r


@pytest.fixture(scope="module")
def room1(room):
    """the room and, as its last mesh, a single triangle"""
    r = copy.deepcopy(room)
    r.add_mesh(np.array([[5.0, 3.4, 2.4], [5.6, 3.6, 2.4], [5.2, 3.5, 3.0]], F), np.array([[0, 1, 2]], np.int32), r.meshes[6]["material"])
    r.triangle_soup()
    return r


# ---- 1
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_gaps_and_a_ragged_end(evplp, room1, builder):
    rm = room1
    last = len(rm.meshes) - 1
    assert len(rm.meshes[last]["idx"]) == 1 and rm.light_mesh not in (0, 2, last)
    targets, weights = {}, {}
    for meshes, T, seed in (([0], 1, 1), ([2], 3, 2), (box_meshes(1), 2, 3), ([last], 64, 4)):
        targets.update(targets_of(rm, meshes, T, amp=0.02 if meshes[0] < 6 else 0.05))
        weights.update({m: weights_of(seed, T) for m in meshes})
    assert sorted(weights) == [0, 2] + box_meshes(1) + [last] and [len(weights[m]) for m in (0, 2, last)] == [1, 3, 64]
    corners = 3 * sum(len(rm.meshes[m]["idx"]) for m in weights)
    assert corners > 256 and corners % 256 != 0, "a ragged last workgroup, and more than one"
    mo = bases(rm, targets, weights)
    assert all(np.abs(mo[m] - rm.meshes[m]["verts"]).max() > 0.01 for m in weights)
    want = by_update(evplp, rm, mo, builder, accel=True)
    assert lit(want) and want["pos"] != fresh(evplp, rm)["pos"], "the motion is not visible"
    with context(evplp, rm, builder) as c:
        set_targets(c, targets)
        same(frame(evplp, c), fresh(evplp, rm, builder), "targets move nothing and mark nothing dirty")
        morph(c, weights)
        c.refit_accel()
        got = with_accel(evplp, c)
        assert c.refit_info()["refits"] == 1
    same(got, want, f"{builder}: meshes 0, 2, a box and the last one by 1, 3, 2 and 64 targets against the update path")
    fb = fresh_build(evplp, rm, mo)
    same({k: got[k] for k in fb}, fb, f"{builder}: against a fresh build of the morphed room")


# ---- 2
def kinds(evplp, room):
    """box 0 morphed only, box 1 morphed under a matrix, box 2 morphed under a pose, box 3 posed only, box 4 by matrix only, box 5 by upload"""
    targets, weights = {}, {}
    for b, T, seed in ((0, 2, 5), (1, 3, 6), (2, 4, 7)):
        targets.update(targets_of(room, box_meshes(b), T)); weights.update({m: weights_of(seed, T) for m in box_meshes(b)})
    skins = {**bend_skin(room, box_meshes(2), 2), **bend_skin(room, box_meshes(3), 3)}
    nb = {**{m: 2 for m in box_meshes(2)}, **{m: 3 for m in box_meshes(3)}}
    pals = {**bend_palette(room, box_meshes(2), (0.0, 35.0)), **bend_palette(room, box_meshes(3), (0.0, 20.0, -30.0), (0.1, -0.1, 0.0))}
    ms = {**{m: rotation_z(room, box_meshes(1), 25.0) for m in box_meshes(1)}, **{m: translation((0.3, -0.2, 0.0)) for m in box_meshes(4)}}
    up = {m: room.meshes[m]["verts"] + np.array([-0.3, 0.25, 0.0], F) for m in box_meshes(5)}
    base = bases(room, targets, weights)
    mo = {m: base[m] for m in box_meshes(0)}
    mo.update({m: evplp.transform_points(ms[m], base[m] if m in base else room.meshes[m]["verts"]) for m in ms})
    mo.update({m: evplp.skin_points(pals[m], skins[m][0], skins[m][1], base[m] if m in base else room.meshes[m]["verts"]) for m in pals})
    mo.update(up)
    return dict(targets=targets, weights=weights, skins=skins, nb=nb, pals=pals, ms=ms, up=up, mo=mo, base=base)


@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_all_kinds_in_one_refit(evplp, room, builder):
    k = kinds(evplp, room)
    want = by_update(evplp, room, k["mo"], builder, accel=True)
    with context(evplp, room, builder) as c:
        set_targets(c, k["targets"]); set_skins(c, k["skins"], k["nb"])
        update(c, k["up"]); morph(c, k["weights"]); transform(c, k["ms"])
        for m, pal in k["pals"].items():
            c.pose_mesh(m, pal)
        c.refit_accel()
        same(with_accel(evplp, c), want, f"{builder}: morphed, morphed under a matrix, morphed under a pose, posed, by matrix, by upload")
        assert c.refit_info()["refits"] == 1
    with context(evplp, room, builder) as c:                                   # the matrix and the pose first, the weights behind them, over two refits
        set_targets(c, k["targets"]); set_skins(c, k["skins"], k["nb"])
        update(c, k["up"]); transform(c, k["ms"])
        for m, pal in k["pals"].items():
            c.pose_mesh(m, pal)
        c.refit_accel()
        morph(c, k["weights"])
        c.refit_accel()
        same(with_accel(evplp, c), want, f"{builder}: weights put in force under a matrix and a pose that a refit had taken")
    fb = fresh_build(evplp, room, k["mo"])
    same({q: want[q] for q in fb}, fb, "the yardstick against a fresh build")


# ---- 3
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_weights_do_not_compose_and_do_not_drift(evplp, room, builder):
    meshes = box_meshes(2)
    T = 3
    targets = targets_of(room, meshes, T)
    skins = bend_skin(room, meshes, 2)
    pa, pb = bend_palette(room, meshes, (0.0, 35.0)), bend_palette(room, meshes, (10.0, -25.0), (0.1, 0.0, 0.0))
    rng = np.random.default_rng(17)
    sets = [rng.uniform(-0.5, 1.5, T).astype(F) for _ in range(100)]
    last = {m: sets[-1] for m in meshes}
    base = bases(room, targets, last)
    want_last = by_update(evplp, room, base, builder)
    want_rest = fresh(evplp, room, builder)
    posed = lambda pal, src: {m: evplp.skin_points(pal[m], skins[m][0], skins[m][1], src[m]) for m in meshes}       # noqa: E731
    rest = {m: room.meshes[m]["verts"] for m in meshes}
    want_a, want_b, want_b_rest = by_update(evplp, room, posed(pa, base), builder), by_update(evplp, room, posed(pb, base), builder), by_update(evplp, room, posed(pb, rest), builder)
    with context(evplp, room, builder) as c:
        set_targets(c, targets)
        for w in sets:
            morph(c, {m: w for m in meshes}); c.refit_accel()
        same(frame(evplp, c), want_last, f"{builder}: a hundred weight sets: the frame is the last one's, applied once to the rest pose")
        assert c.refit_info()["refits"] == 100
        morph(c, {m: sets[3] for m in meshes}); morph(c, last); c.refit_accel()      # (the second call replaces the first before a refit too)
        same(frame(evplp, c), want_last, f"{builder}: two calls, one refit")
        # a pose change alone keeps the morph
        set_skins(c, skins, 2)
        for m in meshes:
            c.pose_mesh(m, pa[m])
        c.refit_accel()
        same(frame(evplp, c), want_a, f"{builder}: a pose on a morphed mesh acts on the morphed base")
        for m in meshes:
            c.pose_mesh(m, pb[m])
        c.refit_accel()
        same(frame(evplp, c), want_b, f"{builder}: another pose alone: the weights stay in force")
        unmorph(c, meshes); c.refit_accel()
        same(frame(evplp, c), want_b_rest, f"{builder}: the weights taken away under a pose: the pose of the rest pose")
        morph(c, last); c.refit_accel()
        same(frame(evplp, c), want_b, f"{builder}: and put back")
        update(c, rest); c.refit_accel()                                       # (forgets pose and weights)
        same(frame(evplp, c), want_rest, f"{builder}: the rest pose by upload")
    with context(evplp, room, builder) as c:
        set_targets(c, targets)
        morph(c, last); c.refit_accel()
        unmorph(c, meshes)
        with pytest.raises(evplp.EvplpError):                                  # dirty: weights were in force
            c.primary(JITTER, clear_light=True)
        c.refit_accel()
        same(frame(evplp, c), want_rest, f"{builder}: NULL, 0 restores the un-morphed frame")
        n = c.refit_info()["refits"]
        unmorph(c, meshes)                                                     # none in force: nothing is dirty
        same(frame(evplp, c), want_rest, "taking away what is not there marks nothing")
        c.refit_accel()
        assert c.refit_info()["refits"] == n


# ---- 4
def test_update_mesh_sets_a_new_rest_pose_keeps_the_targets_and_forgets_the_weights(evplp, room):
    meshes = box_meshes(2)
    targets = targets_of(room, meshes, 3)
    w = {m: weights_of(8, 3) for m in meshes}
    v1 = {m: room.meshes[m]["verts"] * np.array([1, 1, 1.3], F) for m in meshes}
    final = bases(room, targets, w, rest=v1)
    want = by_update(evplp, room, final)
    assert want["pos"] != by_update(evplp, room, bases(room, targets, w))["pos"], "the new rest pose must show"
    with context(evplp, room) as c:
        set_targets(c, targets)
        morph(c, w); c.refit_accel()
        update(c, v1); c.refit_accel()
        same(frame(evplp, c), by_update(evplp, room, v1), "the update forgets the weights")
        for m in meshes:
            assert c.mesh_vertices(m, 2).tobytes() == v1[m].tobytes()
        morph(c, w); c.refit_accel()
        same(frame(evplp, c), want, "morph, update, morph: the same weights morph the new rest pose")
    with context(evplp, room) as c:
        set_targets(c, targets)
        update(c, v1); morph(c, w); c.refit_accel()                            # (a mesh that never was morphed: the rest pose comes from the host)
        same(frame(evplp, c), want, "update then morph in front of one refit")


# ---- 5
def test_new_targets_between_a_morph_and_its_refit(evplp, room):
    meshes = box_meshes(2)
    t3, t2 = targets_of(room, meshes, 3), targets_of(room, meshes, 2, amp=0.07)
    w3, w2 = {m: weights_of(9, 3) for m in meshes}, {m: weights_of(10, 2) for m in meshes}
    want3, want2 = by_update(evplp, room, bases(room, t3, w3)), by_update(evplp, room, bases(room, t2, w2))
    assert want3["pos"] != want2["pos"]
    for warm in (False, True):
        with context(evplp, room) as c:
            set_targets(c, t3)
            if warm:
                morph(c, w3); c.refit_accel()
            morph(c, w3)
            for m in meshes:
                for call in (lambda: c.set_mesh_morph(m, t2[m]), lambda: c.set_mesh_morph(m, None)):
                    with pytest.raises(evplp.EvplpError) as e:
                        call()
                    assert e.value.status == evplp.ERR_INVALID and "weights in force" in str(e.value)
            c.refit_accel()
            same(frame(evplp, c), want3, f"warm {warm}: the refused targets changed nothing")
            unmorph(c, meshes)
            set_targets(c, t2)                                                 # between taking the weights away and the refit
            with pytest.raises(evplp.EvplpError):
                morph(c, w3)                                                   # another target count now
            morph(c, w2); c.refit_accel()
            same(frame(evplp, c), want2, f"warm {warm}: the new targets are used by the next morph")


# ---- 6
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_the_light_morphed(evplp, room, builder):
    lm = room.light_mesh
    v = room.meshes[lm]["verts"]
    x0, x1 = F(v[:, 0].min()), F(v[:, 0].max())
    t = ((v[:, 0] - x0) / (x1 - x0)).astype(F)
    d = np.zeros((2,) + v.shape, F)
    d[0][:, 0] = (t - F(0.5)) * F(0.8); d[0][:, 2] = F(-0.3)                   # stretched along x and lowered
    d[1][:, 2] = t * F(-0.4)                                                  # tilted
    targets, weights = {lm: d}, {lm: np.array([1.0, 0.5], F)}
    mo = bases(room, targets, weights)
    want = fresh_build(evplp, room, mo)
    orig = fresh(evplp, room)
    assert want["metrics"][2] != orig["metrics"][2] and want["records"] != orig["records"]               # the light's area, the light-traced records
    with context(evplp, room, builder) as c:
        set_targets(c, targets); morph(c, weights)
        c.refit_accel()
        assert c.scene_metrics() == want["metrics"]
        same(frame(evplp, c), want, f"{builder}: the light by morph targets against a fresh build")
    same(by_update(evplp, room, mo, builder), want, "the update path")


# ---- 7
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_degenerate_meshes(evplp, builder):
    light, lidx, floor = tiny_scene(9)
    d = np.stack([-floor, np.tile(np.array([0, -0.25, 0], F), (len(floor), 1))]).astype(F)      # target 0 with weight 1 takes every vertex to the origin
    off_w, on_w = np.array([1.0, 0.0], F), np.array([0.0, 1.0], F)
    off_v, on_v = restate_morph(floor, d, off_w), restate_morph(floor, d, on_w)
    assert not off_v.any()
    with tiny_context(evplp, "sah", light, lidx, off_v)[0] as c:
        want_off = tiny_render(evplp, c), c.scene_metrics()
    with tiny_context(evplp, "sah", light, lidx, on_v)[0] as c:
        want_on = tiny_render(evplp, c), c.scene_metrics()
    c, fm = tiny_context(evplp, builder, light, lidx, floor)
    with c:
        c.set_mesh_morph(fm, d)
        c.morph_mesh(fm, off_w)                                                # weights that collapse every triangle switch the mesh off in place
        c.refit_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_off
        c.morph_mesh(fm, on_w)                                                 # the next weights bring it back: every triangle still has its leaf
        c.refit_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_on and want_on[0][0] != want_off[0][0]
        # ... but a tree BUILT while the mesh was off dropped its triangles: weights that give them an area are refused by the refit
        c.morph_mesh(fm, off_w)
        c.build_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_off
        c.morph_mesh(fm, on_w)
        with pytest.raises(evplp.EvplpError) as e:
            c.refit_accel()
        assert e.value.status == evplp.ERR_INVALID and "had no area when the tree was built and has one now" in str(e.value) and "evplp_build_accel" in str(e.value)
        with pytest.raises(evplp.EvplpError):                                 # still dirty
            c.primary((0.0, 0.0), clear_light=True)
        c.build_accel()
        assert (tiny_render(evplp, c), c.scene_metrics()) == want_on


# ---- 8
def test_refusals_and_the_dirty_state(evplp, room):
    L = evplp.lib()
    meshes = box_meshes(0)
    m0 = meshes[0]
    T = 3
    targets = targets_of(room, meshes, T)
    weights = {m: weights_of(11, T) for m in meshes}
    targets[m0][0, 0, 0] = 2.0                                                 # (one delta beyond 1.2: a weight of 3e38 overflows on it)
    d, w = targets[m0], weights[m0]
    n = d.shape[1]
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        mat = c.add_material((0.5, 0.5, 0.5), (0, 0, 0), 0.0)
        c.add_mesh(room.meshes[m0]["verts"], room.meshes[m0]["idx"], mat)
        for call in (lambda: c.set_mesh_morph(0, d), lambda: c.morph_mesh(0, w), lambda: c.morph_mesh(0, None)):
            with pytest.raises(evplp.EvplpError) as e:                        # no accel built
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_build_accel" in str(e.value)
    want = by_update(evplp, room, bases(room, targets, weights))

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
        refused(lambda: c.morph_mesh(m0, w), "no targets yet", "has no morph targets")
        target_cases = {"mesh < 0": (-1, d), "mesh = count": (len(room.meshes), d), "a vertex too few": (m0, d[:, :-1]), "a vertex too many": (m0, np.concatenate([d, d[:, :1]], 1)),
                        "65 targets": (m0, np.zeros((65, n, 3), F)), "delta nan": (m0, edit(d, (2, n - 1, 2), np.nan)), "delta inf": (m0, edit(d, (0, 0, 0), np.inf))}
        for what, args in target_cases.items():
            refused(lambda: c.set_mesh_morph(*args), what)
            same(frame(evplp, c), before, f"{what}: nothing was changed by refused targets: the context renders, and renders the same")
        assert L.evplp_set_mesh_morph(c._h, m0, T, None, n) == evplp.ERR_INVALID and L.evplp_set_mesh_morph(c._h, m0, -1, d.ctypes.data, n) == evplp.ERR_INVALID
        refused(lambda: c.morph_mesh(m0, w), "still no targets", "has no morph targets")
        set_targets(c, targets)
        same(frame(evplp, c), before, "targets mark nothing dirty")
        over_w = edit(w, 0, 3e38)                                              # finite, but 3e38 x a delta overflows
        assert np.isfinite(over_w).all() and np.abs(d[0]).max() > 1.2
        morph_cases = {"mesh < 0": (-1, w), "mesh = count": (len(room.meshes), w), "a mesh without targets": (box_meshes(1)[0], w), "a weight too few": (m0, w[:-1]),
                       "a weight too many": (m0, np.concatenate([w, w[:1]])), "weight nan": (m0, edit(w, 1, np.nan)), "weight inf": (m0, edit(w, 2, -np.inf)),
                       "a final coordinate that is not finite": (m0, over_w)}
        for what, args in morph_cases.items():
            refused(lambda: c.morph_mesh(*args), what)
            same(frame(evplp, c), before, f"{what}: nothing was marked by a refused morph")
        refused(lambda: c.morph_mesh(m0, over_w), "over", "not finite under the weights")
        assert L.evplp_morph_mesh(c._h, m0, None, T) == evplp.ERR_INVALID
        same(frame(evplp, c), before, "a null pointer with a count: nothing was marked")
        # a final coordinate: the base is finite, the matrix in force takes it out of range
        m1 = box_meshes(1)[0]
        assert np.abs(room.meshes[m1]["verts"]).max() < 50
        c.set_mesh_morph(m1, np.ones((1,) + room.meshes[m1]["verts"].shape, F))
        c.transform_mesh(m1, np.array([1e36, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F))                          # finite on the rest pose: accepted
        refused(lambda: c.morph_mesh(m1, np.array([1e3], F)), "a finite base, but not under the matrix in force", "matrix in force")
        c.update_mesh(m1, room.meshes[m1]["verts"]); c.refit_accel()           # (forgets the matrix: no refit ever saw it)
        same(frame(evplp, c), before, "the rest pose given again")
        n0 = c.refit_info()["refits"]
        morph(c, weights)
        cam = c.camera()
        fp = evplp.frame_params(camera_pos=list(cam.origin), num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
        for call in (lambda: c.primary(JITTER, clear_light=True), lambda: c.trace_light_paths(7), lambda: c.gather_vpl(fp), lambda: c.gather_lvc(fp),
                     lambda: c.splat_photons(fp, clear=True), lambda: c.path_trace(list(cam.origin), 5, 3)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value) and "evplp_build_accel" in str(e.value)
        refused(lambda: c.morph_mesh(m0, over_w), "a refusal on a dirty context leaves it dirty, and as it was")
        c.refit_accel()
        same(frame(evplp, c), want, "after the refusals")
        assert c.refit_info()["refits"] == n0 + 1


# ---- 9
def test_rebuilds_keep_the_targets_and_the_weights(evplp, room):
    meshes = box_meshes(2)
    targets = targets_of(room, meshes, 3)
    skins = bend_skin(room, meshes, 2)
    wa, wb = {m: weights_of(12, 3) for m in meshes}, {m: weights_of(13, 3) for m in meshes}
    pa, pb = bend_palette(room, meshes, (0.0, 35.0)), bend_palette(room, meshes, (10.0, -25.0), (0.1, 0.0, 0.0))
    posed = lambda pal, src: {m: evplp.skin_points(pal[m], skins[m][0], skins[m][1], src[m]) for m in meshes}       # noqa: E731
    ba, bb = bases(room, targets, wa), bases(room, targets, wb)
    want = {"a": by_update(evplp, room, ba), "b": by_update(evplp, room, bb), "a under pa": by_update(evplp, room, posed(pa, ba)), "a under pb": by_update(evplp, room, posed(pb, ba)),
            "b under pb": by_update(evplp, room, posed(pb, bb))}
    with context(evplp, room) as c:
        set_targets(c, targets); set_skins(c, skins, 2)
        c.set_refit_policy(1e-3, BUILDERS["gpu"])                             # any refit costs more than a thousandth of the built tree: it rebuilds
        morph(c, wa); c.refit_accel()
        assert c.accel_quality()["last_action"] == 2 and c.accel_quality()["policy_rebuilds"] == 1
        same(frame(evplp, c), want["a"], "A, policy rebuild")
        morph(c, wb); c.refit_accel()
        assert c.accel_quality()["policy_rebuilds"] == 2
        same(frame(evplp, c), want["b"], "B after a policy rebuild starts from the rest pose, with the kept targets")
        c.set_refit_policy(0.0)
        morph(c, wa); c.refit_accel()                                         # a plain refit of the rebuilt tree: the kernel, the deltas sent again
        assert c.accel_quality()["policy_rebuilds"] == 2
        same(frame(evplp, c), want["a"], "A by the kernel after the rebuilds")
    with context(evplp, room) as c:
        set_targets(c, targets); set_skins(c, skins, 2)
        morph(c, wa)
        for m in meshes:
            c.pose_mesh(m, pa[m])
        c.build_accel()                                                        # the full rebuild on a context dirty by weights and pose
        same(frame(evplp, c), want["a under pa"], "build_accel on a context dirty by weights and pose")
        for m in meshes:
            c.pose_mesh(m, pb[m])                                              # the pose alone: the weights' effect survived the rebuild
        c.refit_accel()
        same(frame(evplp, c), want["a under pb"], "a pose after build_accel acts on the morphed base")
        morph(c, wb); c.refit_accel()
        same(frame(evplp, c), want["b under pb"], "weights after build_accel: the targets survived it")
        assert c.refit_info()["refits"] == 2


@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_rotations_on(evplp, room, builder):
    k = kinds(evplp, room)
    with context(evplp, room, builder) as c:
        c.set_refit_rotations(1)
        update(c, k["mo"]); c.refit_accel()
        want = with_accel(evplp, c)
        want_rot = c.rotation_info()
    with context(evplp, room, builder) as c:
        c.set_refit_rotations(1)
        set_targets(c, k["targets"]); set_skins(c, k["skins"], k["nb"])
        update(c, k["up"]); morph(c, k["weights"]); transform(c, k["ms"])
        for m, pal in k["pals"].items():
            c.pose_mesh(m, pal)
        c.refit_accel()
        same(with_accel(evplp, c), want, f"{builder}: a morphed refit with rotations against the same setting over the update path")
        assert c.rotation_info() == want_rot
    fb = fresh_build(evplp, room, k["mo"])
    same({q: want[q] for q in fb}, fb, f"{builder}: with rotations the frame stays the fresh build's")


# ---- 10
def test_groups(evplp, room):
    k = kinds(evplp, room)
    mo = k["mo"]
    with context(evplp, room) as c:
        update(c, mo); c.refit_accel()
        _, total, _ = c.scene_metrics()
        fp = group_frame_params(evplp, room, total, 7)
        c.clear_accumulators()
        c.primary(JITTER, clear_light=True); c.trace_light_paths(7); c.gather_vpl(fp); c.splat_photons(fp)
        want = c.resolve(1.0, 1.0, 1.0)[:H].tobytes()
    assert np.frombuffer(want, F).max() > 0
    m0 = box_meshes(0)[0]

    def move(g):
        set_targets(g, k["targets"]); set_skins(g, k["skins"], k["nb"])
        update(g, k["up"]); morph(g, k["weights"]); transform(g, k["ms"])
        for m, pal in k["pals"].items():
            g.pose_mesh(m, pal)
    with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True) as g:
        for r in range(2):
            room.upload(g.rank(r))
        for call in (lambda: g.set_mesh_morph(len(room.meshes), k["targets"][m0]), lambda: g.set_mesh_morph(m0, k["targets"][m0][:, :-1]),
                     lambda: g.morph_mesh(m0, k["weights"][m0])):              # (the last: no targets yet) refused on the caller's thread: the group stays usable
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID
        set_targets(g, k["targets"])
        with pytest.raises(evplp.EvplpError) as e:
            g.morph_mesh(m0, k["weights"][m0][:1])
        assert e.value.status == evplp.ERR_INVALID
        move(g)
        with pytest.raises(evplp.EvplpError) as e:
            g.primary(JITTER, 1)
        assert e.value.status == evplp.ERR_INVALID and "evplp_group_refit_accel" in str(e.value)
        g.refit_accel()
        assert all(g.rank(r).refit_info()["refits"] == 1 for r in range(2))
        assert group_frame(evplp, g, room, total) == want, "2 ranks, strips"
        for r in range(2):
            assert g.rank(r).mesh_vertices(m0, 2).tobytes() == k["base"][m0].tobytes()
    frames = []
    for by_morph in (False, True):
        with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True, partition="iterations") as g:
            for r in range(2):
                room.upload(g.rank(r))
            if by_morph:
                move(g)
            else:
                update(g, mo)
            g.refit_accel()
            frames.append(group_frame(evplp, g, room, total, n_iter=2))
    assert frames[0] == frames[1] and np.frombuffer(frames[0], np.uint8).any()


# ---- 11: a "weights" track of the technique JSON against plain renders of scenes whose OBJ file holds the moved vertices
BOX_LO, BOX_HI = (11.0, -3.0, 0.0), (13.0, -1.0, 1.5)
FRAMES = 3


def _targets_of(p):
    """two targets of the extra box as functions of the position: the top swells, the box leans"""
    t = (p[:, 2] / F(BOX_HI[2])).astype(F)
    ctr = np.array([12.0, -2.0, 0.0], F)
    d0 = (p - ctr) * F(0.3) * t[:, None]; d0[:, 2] = 0
    d1 = np.zeros_like(p); d1[:, 0] = t * F(0.5); d1[:, 2] = t * F(0.2)
    return np.stack([d0, d1]).astype(F)


def _weights(f):
    return np.array([0.4 * (f + 1), 1.0 - 0.75 * f], F)


def _bend_of(p):
    t = (p[:, 2] / F(BOX_HI[2])).astype(F)
    idx = np.tile(np.array([0, 1, 0, 0], np.int32), (len(p), 1))
    return idx, np.stack([F(1) - t, t, np.zeros_like(t), np.zeros_like(t)], 1).astype(F)


def _palette(f):
    m = np.eye(3, 4, dtype=F); m[0, 1] = 0.2 * (f + 1); m[:, 3] = (0.3 * (f + 1), -0.4, 0.25 * f)
    return np.stack([IDENTITY, m.reshape(12)]).astype(F)


def _scene_dir(evplp, tmp_path, name, move=None):
    """a directory with the room and one more object, a box; move(points) -> points rewrites the box's `v` lines"""
    d = tmp_path / name
    d.mkdir()
    src = tmp_path / "src"
    if not src.exists():
        src.mkdir()
        evplp.synth_scene(str(src), "room", 600, 1, W, H)
        _box_obj(str(src / "extra.obj"), BOX_LO, BOX_HI, "obj3")
    for f in ("room.mtl", "room_lights.obj", "room.obj", "extra.obj"):
        shutil.copy(src / f, d / f)
    if move is not None:
        lines = _obj_lines(str(src / "extra.obj"))
        rows = [i for i, ln in enumerate(lines) if ln.startswith("v ")]
        pts = np.array([[float(t) for t in lines[i].split()[1:4]] for i in rows], np.float64).astype(F)
        for i, p in zip(rows, move(pts)):
            lines[i] = "v %.9g %.9g %.9g" % (float(p[0]), float(p[1]), float(p[2]))
        open(d / "extra.obj", "w").write("\n".join(lines))
    root = json.load(open(src / "room.json"))
    root["scene"] = ["room.obj", "extra.obj"]
    fam = root.pop("photonfam")
    fam.update({"numMaxIteration": 2, "deterministic": True, "radiusPercentage": 0.02, "run": {"photonSplat": True}, "rngOffset": 3, "timeLimitMs": 1e9})
    root["photonfam"] = fam
    (d / "room.json").write_text(json.dumps(root))
    return d


@pytest.mark.parametrize("beside", ["alone", "poses"])
def test_weights_track(evplp, tmp_path, beside):
    def moved(f):
        def move(pts):
            base = restate_morph(pts, _targets_of(pts), _weights(f))
            return base if beside == "alone" else evplp.skin_points(_palette(f), *_bend_of(pts), base)
        return move
    want = []
    for f in range(FRAMES):
        d = _scene_dir(evplp, tmp_path, f"ref{f}", moved(f))
        evplp.render_json(str(d / "room.json"))
        want.append({n: (d / n).read_bytes() for n in OUTPUTS["photonfam"]})
    assert want[0] != want[1] and want[1] != want[2], "the motion is not visible"
    d = _scene_dir(evplp, tmp_path, "anim")
    # vertex v is the loader's numbering: the queries return it
    with evplp.Context(W, H, NPATHS, NPATHS, P) as c:
        c.load_scene_json(str(d / "room.json"))
        box = [m for m in range(c.mesh_count()) if c.mesh_info(m)["nverts"] == 8 and (c.mesh_vertices(m) >= np.array(BOX_LO, F)).all() and (c.mesh_vertices(m) <= np.array(BOX_HI, F)).all()]
        assert len(box) == 1 and c.mesh_info(box[0])["ntris"] == 12
        verts = c.mesh_vertices(box[0])
    fl = lambda a: [float(x) for x in a]                                        # noqa: E731
    track = {"mesh": box[0], "morph": {"targets": [[fl(v) for v in t] for t in _targets_of(verts)]}, "weights": [fl(_weights(f)) for f in range(FRAMES)]}
    if beside == "poses":
        idx, w = _bend_of(verts)
        track.update({"skin": {"bones": 2, "indices": idx.tolist(), "weights": [fl(r) for r in w]}, "poses": [[fl(m) for m in _palette(f)] for f in range(FRAMES)]})
    evplp.render_json(str(d / "room.json"), json.dumps({"animation": {"frames": FRAMES, "tracks": [track]}}))
    for f in range(FRAMES):
        for name in OUTPUTS["photonfam"]:
            stem, ext = name.rsplit(".", 1)
            p = d / f"{stem}_f{f:04d}.{ext}"
            assert p.exists(), sorted(q.name for q in d.iterdir())
            assert p.read_bytes() == want[f][name], f"{beside}: frame {f}, {name} differs from a plain render of the moved scene"


# ---- 12
def test_temporal(evplp):
    import test_gpu_temporal as tt
    box = tt.make_box()
    meshes = tt.BOX_MESHES
    targets = targets_of(box, meshes, 2, amp=0.06)
    w = np.array([1.0, 0.5], F)
    out = []
    for by_morph in (False, True):
        with evplp.Context(tt.W, tt.H, 1, 1, 1) as c:
            box.upload(c); c.noise_track(True); c.temporal_enable(True)
            if by_morph:
                set_targets(c, targets)
            tt.render(evplp, c, box.cam_origin, 0)
            imgs = [c.denoise_temporal(1.0 / tt.ITERS)[0].tobytes()]
            for m in meshes:
                c.morph_mesh(m, w) if by_morph else c.update_mesh(m, restate_morph(box.meshes[m]["verts"], targets[m], w))
            c.refit_accel()
            tt.render(evplp, c, box.cam_origin, 1)
            img, info = c.denoise_temporal(1.0 / tt.ITERS)
            imgs.append(img.tobytes())
            out.append((imgs, info, tuple(c.temporal_download(k).tobytes() for k in range(3))))
    assert out[1][1]["reprojected"] > 0 and out[1][1]["frames_since_reset"] == 2
    assert out[0][0][0] != out[0][0][1], "the motion is not visible"
    assert out[1][0] == out[0][0] and out[1][1] == out[0][1] and out[1][2] == out[0][2], "two frames of a morphed box against the same frames through evplp_update_mesh"


# ---- 13
def test_queries(evplp, room):
    m0 = box_meshes(2)[1]
    targets = targets_of(room, [m0], 3); w = weights_of(14, 3)
    skins = bend_skin(room, [m0], 2); pal = bend_palette(room, [m0], (0.0, 35.0), (0.1, 0.0, 0.2))[m0]
    rest = room.meshes[m0]["verts"]
    base = restate_morph(rest, targets[m0], w)
    posed = evplp.skin_points(pal, skins[m0][0], skins[m0][1], base)
    mat = rotation_z(room, [m0], 25.0)
    L = evplp.lib()
    with context(evplp, room) as c:
        out = np.zeros((64, 3), F)
        assert L.evplp_mesh_vertices(c._h, m0, 2, out.ctypes.data, 64) == evplp.ERR_INVALID and not out.any(), "a mesh without targets has no morphed base"
        set_targets(c, targets); set_skins(c, skins, 2)
        q = lambda: tuple(c.mesh_vertices(m0, k).tobytes() for k in range(3))   # noqa: E731
        assert q() == (rest.tobytes(),) * 3
        c.morph_mesh(m0, w)
        assert q() == (base.tobytes(), rest.tobytes(), base.tobytes())
        c.pose_mesh(m0, pal)
        assert q() == (posed.tobytes(), rest.tobytes(), base.tobytes())
        c.refit_accel()
        assert q() == (posed.tobytes(), rest.tobytes(), base.tobytes())
        c.transform_mesh(m0, mat)
        assert q() == (evplp.transform_points(mat, base).tobytes(), rest.tobytes(), base.tobytes())
        c.morph_mesh(m0, None)
        assert q() == (evplp.transform_points(mat, rest).tobytes(), rest.tobytes(), rest.tobytes())
        c.refit_accel()
        c.morph_mesh(m0, w); c.update_mesh(m0, posed); c.refit_accel()         # a new rest pose: the weights are forgotten
        assert q() == (posed.tobytes(),) * 3
        assert L.evplp_mesh_vertices(c._h, m0, 3, out.ctypes.data, 64) == evplp.ERR_INVALID and L.evplp_mesh_vertices(c._h, m0, 2, out.ctypes.data, len(rest) - 1) == evplp.ERR_INVALID
        assert not out.any()


# ---- a context that never morphs launches and allocates nothing new; one that does, frees it with the scene
def test_a_mesh_without_weights_behaves_as_before(evplp, room):
    k = kinds(evplp, room)
    mo = {m: v for m, v in k["mo"].items() if m in box_meshes(3) + box_meshes(4) + box_meshes(5)}
    want = by_update(evplp, room, mo)
    with context(evplp, room) as c:
        set_targets(c, k["targets"]); set_skins(c, k["skins"], k["nb"])       # targets attached, never any weights
        update(c, k["up"]); transform(c, {m: k["ms"][m] for m in box_meshes(4)})
        for m in box_meshes(3):
            c.pose_mesh(m, k["pals"][m])
        c.refit_accel()
        same(frame(evplp, c), want, "targets without weights: the refit is the one it was")
