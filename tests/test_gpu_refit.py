"""Scenes that move: evplp_update_mesh + evplp_refit_accel against a FRESH build of the moved scene.  Visibility and closest hit are exact
predicates over the triangles and boxes only have to be conservative (test_gpu_bvh.py holds every builder's frame to the same bytes), so a
refit -- same topology, same leaf assignment, new operands and boxes -- must give a fresh build's frame bit for bit, whatever builder made
the tree; and the structure itself is restated in numpy fp32: operands, the exact min / max under every child padded once, four-wide nodes."""
import copy
import math

import numpy as np
import pytest

import scenes

pytestmark = pytest.mark.gpu

W, H = 96, 64
NPATHS, P = 64, 4
BUILDERS = {"lbvh": 0, "sah": 1, "sbvh": 2, "gpu": 3}
JITTER = (0.002, -0.001)
F = np.float32


@pytest.fixture(scope="module")
def room():
    return scenes.box_room(seed=11, n_boxes=7, tess=3, aspect=W / H)


def box_meshes(b):
    return list(range(6 + 6 * b, 12 + 6 * b))


# ---- motions: {mesh: new vertices}, computed once in numpy fp32; the same arrays feed update_mesh and the fresh build
def translate(room, meshes, d):
    return {m: room.meshes[m]["verts"] + np.asarray(d, F) for m in meshes}


def rotate_z(room, meshes, degrees):
    """about the vertical (z) through the centre of the meshes' bounding box"""
    allv = np.concatenate([room.meshes[m]["verts"] for m in meshes])
    ctr = F(0.5) * (allv.min(0) + allv.max(0))
    c, s = F(math.cos(math.radians(degrees))), F(math.sin(math.radians(degrees)))
    out = {}
    for m in meshes:
        v = room.meshes[m]["verts"]
        x, y = v[:, 0] - ctr[0], v[:, 1] - ctr[1]
        out[m] = np.stack([ctr[0] + (c * x - s * y), ctr[1] + (s * x + c * y), v[:, 2]], axis=1).astype(F)
    return out


def scale_z(room, meshes, k):
    return {m: room.meshes[m]["verts"] * np.array([1, 1, k], F) for m in meshes}


def moved_room(room, motion):
    r = copy.deepcopy(room)
    for m, v in motion.items():
        assert v.dtype == F and v.shape == r.meshes[m]["verts"].shape
        r.meshes[m]["verts"] = v.copy()
    r.triangle_soup()
    return r


def motion_a(room):
    mo = {}
    mo.update(translate(room, box_meshes(0), (0.35, -0.2, 0.0)))
    mo.update(rotate_z(room, box_meshes(2), 25.0))
    mo.update(scale_z(room, box_meshes(4), 1.4))
    assert len(mo) == 18
    return mo


def motion_b(room, room_a):
    """on top of A: box 0 back to where it was, box 5 moved"""
    mo = {m: room.meshes[m]["verts"].copy() for m in box_meshes(0)}
    mo.update(translate(room_a, box_meshes(5), (-0.3, 0.25, 0.0)))
    return mo


def motion_light(room):
    lm = room.light_mesh
    v = room.meshes[lm]["verts"]
    cx = F(0.5) * (v[:, 0].min() + v[:, 0].max())
    nv = v.copy()
    nv[:, 0] = cx + (v[:, 0] - cx) * F(1.2)
    nv[:, 2] = v[:, 2] - F(0.4)
    wall = room.meshes[1]["verts"].copy()                    # the shell's +x face (x = 10)
    assert np.all(wall[:, 0] == 10.0)
    wall[:, 0] += F(0.5)
    return {lm: nv.astype(F), 1: wall}


def apply(c, motion):
    for m, v in motion.items():
        c.update_mesh(m, v)


# ---- the frame: test_gpu_bvh.py's render on an open context, plus an LVC gather and an accumulating path trace (the four-wide walks)
def render(evplp, c):
    c.clear_accumulators()
    c.primary(JITTER, clear_light=True)
    c.trace_light_paths(7)
    cam = c.camera()
    _, total, _ = c.scene_metrics()
    fp = evplp.frame_params(camera_pos=list(cam.origin), mis_mode=1, pdf_mc=0.4, clamping_value=1.0 / total, photon_radius=0.3,
                            num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P, rng_seed=7)
    out = {}
    for k, b in (("pos", evplp.BUF_GBUF_POSITION), ("nrm", evplp.BUF_GBUF_NORMAL), ("dif", evplp.BUF_GBUF_DIFFUSE), ("phg", evplp.BUF_GBUF_PHONG), ("light", evplp.BUF_LIGHT)):
        out[k] = c.download(b)[:H].tobytes()
    out["records"] = c.download(evplp.BUF_RECORDS).tobytes()
    c.gather_vpl(fp)
    out["vpl"] = c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes()
    st = c.pass_stats(evplp.PASS_GATHER_VPL)
    out["vpl rays"], out["vpl pairs"] = st["rays"], st["pairs"]
    c.gather_lvc(fp)
    out["lvc"] = c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes()
    st = c.pass_stats(evplp.PASS_GATHER_LVC)
    out["lvc rays"], out["lvc pairs"] = st["rays"], st["pairs"]
    c.path_trace(list(cam.origin), 5, 3, accumulate=True)
    out["lvc + pt"] = c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes()
    c.splat_photons(fp, clear=True)
    out["photon"] = c.download(evplp.BUF_PHOTON_ACCUM)[:H].tobytes()
    return out


def fresh(evplp, sd, builder="sah"):
    with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True) as c:
        sd.upload(c)
        r = render(evplp, c)
        r["metrics"] = c.scene_metrics()
    return r


def same(got, want, what):
    for k, v in want.items():
        if k != "metrics":
            assert got[k] == v, f"{what}: {k} differs from the fresh build's"


def lit(r):
    return all(np.frombuffer(r[k], F).max() > 0 for k in ("vpl", "lvc", "lvc + pt", "photon")) and r["vpl rays"] > 0 and r["lvc rays"] > 0


@pytest.fixture(scope="module")
def rooms(room):
    a = moved_room(room, motion_a(room))
    return {"a": a, "b": moved_room(a, motion_b(room, a)), "light": moved_room(room, motion_light(room))}


@pytest.fixture(scope="module")
def fresh_frames(evplp, room, rooms):
    """the references, rendered once: a fresh SAH build of every scene, and the device LBVH of the moved ones (the precondition)"""
    out = {"orig": fresh(evplp, room)}
    for k, sd in rooms.items():
        out[k] = fresh(evplp, sd)
        out[k + " gpu"] = fresh(evplp, sd, "gpu")
    return out


# ---- 1
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_refit_equals_a_fresh_build(evplp, room, rooms, fresh_frames, builder):
    for k in ("a", "b"):
        assert lit(fresh_frames[k]), "the moved room renders black"
        same(fresh_frames[k + " gpu"], fresh_frames[k], f"PRECONDITION (motion {k}): fresh device LBVH vs fresh SAH of the moved room -- the motion must change, not the comparison")
        assert fresh_frames[k]["pos"] != fresh_frames["orig"]["pos"] and fresh_frames[k]["vpl"] != fresh_frames["orig"]["vpl"], "the motion is not visible"
    assert fresh_frames["a"]["pos"] != fresh_frames["b"]["pos"]
    with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True) as c:
        room.upload(c)
        apply(c, motion_a(room))
        c.refit_accel()
        same(render(evplp, c), fresh_frames["a"], f"{builder}, motion A")
        info = c.refit_info()
        assert info["refits"] == 1 and 1 <= info["levels"] <= c.accel_info()["depth"], (info, c.accel_info())
        apply(c, motion_b(room, rooms["a"]))
        c.refit_accel()
        same(render(evplp, c), fresh_frames["b"], f"{builder}, motion B (second refit)")
        assert c.refit_info()["refits"] == 2 and c.refit_info()["levels"] == info["levels"]


# ---- 2
@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_the_light_and_the_bounds_move(evplp, room, rooms, fresh_frames, builder):
    want = fresh_frames["light"]
    same(fresh_frames["light gpu"], want, "PRECONDITION: fresh device LBVH vs fresh SAH of the room with the moved light")
    assert want["metrics"][0] != fresh_frames["orig"]["metrics"][0] and want["metrics"][2] != fresh_frames["orig"]["metrics"][2]     # radius and light area
    with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True) as c:
        room.upload(c)
        pad0 = c.debug_accel(5)
        apply(c, motion_light(room))
        c.refit_accel()
        assert c.scene_metrics() == want["metrics"]
        assert c.debug_accel(5) > pad0, "the pad follows the scene bounds"
        same(render(evplp, c), want, f"{builder}, light and wall moved")


# ---- 3: the structure itself, restated in numpy fp32
def set_box(lo, hi, pad):
    lo, hi = (lo - pad).astype(F), (hi + pad).astype(F)
    c = (F(0.5) * (lo + hi)).astype(F)
    h = np.maximum(hi - c, c - lo).astype(F)
    h = ((h + np.abs(h) * F(1e-6)).astype(F) + F(1e-30)).astype(F)
    return c, h


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_the_structure_itself(evplp, room, rooms, builder):
    soup = rooms["a"].triangle_soup()[0]                                     # (ntri, 9) fp32, mesh order
    with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True) as c:
        room.upload(c)
        before = {w: c.debug_accel(w).copy() for w in (0, 3)}
        apply(c, motion_a(room))
        c.refit_accel()
        nodes, leaves, flat, ti, nodes4, pad = (c.debug_accel(w) for w in range(6))
    assert pad.dtype == F and pad > 0
    NO = evplp.NO_CHILD
    # topology and leaf assignment are the build's
    for s in ("c0", "c1"):
        assert np.array_equal(nodes[s], before[0][s])
    assert np.array_equal(ti, before[3])
    # operands: e0 = p1 - p0, e1 = p0 - p2, n = cross(e1, e0), every operation rounded to fp32
    live = ti >= 0
    assert live.sum() >= soup.shape[0] - 2 and np.all(ti[~live] == -1)
    v = soup[ti[live]]
    p0, e0, e1 = v[:, 0:3], v[:, 3:6] - v[:, 0:3], v[:, 0:3] - v[:, 6:9]
    n = np.stack([e1[:, 1] * e0[:, 2] - e1[:, 2] * e0[:, 1], e1[:, 2] * e0[:, 0] - e1[:, 0] * e0[:, 2], e1[:, 0] * e0[:, 1] - e1[:, 1] * e0[:, 0]], axis=1)
    assert all(a.dtype == F for a in (p0, e0, e1, n))
    for name, want in (("p0", p0), ("e0", e0), ("e1", e1), ("n", n)):
        pair = leaves["pair"][name].transpose(0, 1, 3, 2).reshape(-1, 3)    # [block][pair][component][half] -> slot = 4 block + 2 pair + half
        for layout, got in (("flat", flat[name]), ("pair", pair)):
            assert np.array_equal(bits(got[live]), bits(want)), f"{name} ({layout} layout)"
            assert not bits(got[~live]).any(), f"{name} ({layout} layout): a dead slot is not zero"
    # boxes: the exact min / max of the vertices under every child, padded once
    height, order, begin = evplp.refit_levels(nodes)
    assert len(order) == len(nodes)
    lo, hi = np.zeros((len(nodes), 3), F), np.zeros((len(nodes), 3), F)
    checked = 0
    for i in order:
        blo, bhi = np.full(3, 3.0e38, F), np.full(3, -3.0e38, F)
        for s, ch in enumerate((int(nodes[i]["c0"]), int(nodes[i]["c1"]))):
            if ch == NO:
                assert np.all(nodes[i]["ctr"][:, s] == 0) and np.all(nodes[i]["hal"][:, s] == F(-3.0e38))
                continue
            if ch >= 0:
                clo, chi = lo[ch], hi[ch]
            else:
                blk, cnt = (~ch) >> 2, ((~ch) & 3) + 1
                tris = ti[4 * blk:4 * blk + cnt]
                pts = soup[tris[tris >= 0]].reshape(-1, 3)
                clo, chi = pts.min(0), pts.max(0)
            ctr, hal = set_box(clo, chi, pad)
            assert np.array_equal(bits(nodes[i]["ctr"][:, s]), bits(ctr)) and np.array_equal(bits(nodes[i]["hal"][:, s]), bits(hal)), (i, s, ch)
            blo, bhi = np.minimum(blo, clo), np.maximum(bhi, chi)
            checked += 1
        lo[i], hi[i] = blo, bhi
    assert checked >= len(nodes)
    # four-wide nodes: node4_kernel restated on the node array
    ctr, hal = nodes["ctr"], nodes["hal"]
    for i in range(len(nodes)):
        child = np.full(4, NO, np.int64); wlo = np.full((3, 4), 3.0e38, F); whi = np.full((3, 4), -3.0e38, F)
        for s, ch in enumerate((int(nodes[i]["c0"]), int(nodes[i]["c1"]))):
            if ch >= 0:
                child[2 * s], child[2 * s + 1] = nodes[ch]["c0"], nodes[ch]["c1"]
                wlo[:, 2 * s:2 * s + 2], whi[:, 2 * s:2 * s + 2] = ctr[ch] - hal[ch], ctr[ch] + hal[ch]
            elif ch != NO:
                child[2 * s] = ch
                wlo[:, 2 * s], whi[:, 2 * s] = ctr[i][:, s] - hal[i][:, s], ctr[i][:, s] + hal[i][:, s]
        assert np.array_equal(nodes4[i]["child"], child), i
        assert np.array_equal(bits(nodes4[i]["lo"]), bits(wlo)) and np.array_equal(bits(nodes4[i]["hi"]), bits(whi)), i
        assert not nodes4[i]["pad"].any()


# ---- 4, 5: tiny trees and degenerate triangles (test_gpu_bvh.py's tiny scenes)
def tiny_scene(ntri):
    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F)
    light = quad + np.array([0, 2.0, 0], F)
    lidx = np.array([[0, 1, 2], [0, 2, 3]][:2 if ntri else 1], np.int32)
    fl = []
    for k in range(ntri):
        x = -1.0 + 2.0 * k / ntri
        fl.append([[x, -1.0, -1.0], [x + 2.0 / ntri, -1.0, -1.0], [x + 1.0 / ntri, -1.0, 1.0]])
    fl.append([[0, -1, 0], [0, -1, 0], [0, -1, 0]])                           # the degenerate one: dropped by every builder
    return light, lidx, np.array(fl, F).reshape(-1, 3)


def tiny_context(evplp, builder, light, lidx, floor):
    c = evplp.Context(32, 32, 16, 16, 4, bvh_builder=BUILDERS[builder])
    m = c.add_material((0.6, 0.6, 0.6), (0.0, 0.0, 0.0), 1.0)
    lm = c.add_mesh(light, lidx, m)
    fm = c.add_mesh(floor, np.arange(len(floor), dtype=np.int32).reshape(-1, 3), m)
    c.set_arealight(lm, (10.0, 10.0, 10.0, 0.0))
    c.set_camera((0.0, 0.5, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.9, 1.0)
    c.build_accel()
    return c, fm


def tiny_render(evplp, c):
    c.primary((0.0, 0.0), clear_light=True)
    c.trace_light_paths(1)
    return tuple(c.download(b).tobytes() for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_RECORDS))


@pytest.mark.parametrize("builder", ["sah", "gpu"])
@pytest.mark.parametrize("ntri", [0, 1, 2, 4, 9])
def test_tiny_trees(evplp, ntri, builder):
    light, lidx, floor = tiny_scene(ntri)
    lowered = floor - np.array([0, 0.25, 0], F)
    with tiny_context(evplp, "sah", light, lidx, lowered)[0] as c:
        want = tiny_render(evplp, c)
    c, fm = tiny_context(evplp, builder, light, lidx, floor)
    with c:
        orig = tiny_render(evplp, c)
        c.update_mesh(fm, lowered)
        c.refit_accel()
        assert tiny_render(evplp, c) == want
        assert c.refit_info()["levels"] >= 1
    assert np.frombuffer(want[0], F).any() or ntri == 0, "the floor should be visible"
    assert want[0] != orig[0] or ntri == 0, "lowering the floor should show"


@pytest.mark.parametrize("builder", ["sah", "gpu"])
def test_degenerate_triangles(evplp, builder):
    light, lidx, floor = tiny_scene(9)
    collapsed = floor.copy()
    collapsed[12:15] = collapsed[12]                                         # floor triangle 4 becomes a point: a fresh build drops it
    with tiny_context(evplp, "sah", light, lidx, collapsed)[0] as c:
        want = tiny_render(evplp, c)
    revived = floor.copy()
    revived[27:30] = np.array([[-0.5, -0.5, -0.5], [0.5, -0.5, -0.5], [0.0, -0.5, 0.5]], F)     # the dropped triangle gets an area
    with tiny_context(evplp, "sah", light, lidx, revived)[0] as c:
        want_revived = tiny_render(evplp, c)
    c, fm = tiny_context(evplp, builder, light, lidx, floor)
    with c:
        orig = tiny_render(evplp, c)
        c.update_mesh(fm, collapsed)
        c.refit_accel()
        assert tiny_render(evplp, c) == want and want[0] != orig[0]
        c.update_mesh(fm, revived)
        with pytest.raises(evplp.EvplpError) as e:
            c.refit_accel()
        assert e.value.status == evplp.ERR_INVALID and "evplp_build_accel" in str(e.value)
        with pytest.raises(evplp.EvplpError) as e:                            # still dirty
            c.primary((0.0, 0.0), clear_light=True)
        assert e.value.status == evplp.ERR_INVALID
        assert c.refit_info()["refits"] == 1
        c.build_accel()
        assert tiny_render(evplp, c) == want_revived and want_revived[0] != want[0]


# ---- 6
def test_refusals_and_the_dirty_state(evplp, room, fresh_frames):
    L = evplp.lib()
    mo = motion_a(room)
    m0 = box_meshes(0)[0]
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        mat = c.add_material((0.5, 0.5, 0.5), (0, 0, 0), 0.0)
        c.add_mesh(room.meshes[0]["verts"], room.meshes[0]["idx"], mat)
        with pytest.raises(evplp.EvplpError) as e:                            # no accel built
            c.update_mesh(0, room.meshes[0]["verts"])
        assert e.value.status == evplp.ERR_INVALID
        with pytest.raises(evplp.EvplpError):
            c.refit_accel()
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        room.upload(c)
        before = render(evplp, c)
        same(before, fresh_frames["orig"], "the unmoved room")
        good = mo[m0]
        bad_nan, bad_inf = good.copy(), good.copy()
        bad_nan[3, 1] = np.nan; bad_inf[0, 2] = np.inf
        for args in ((-1, good), (len(room.meshes), good), (m0, good[:-1]), (m0, np.concatenate([good, good[:1]])), (m0, bad_nan), (m0, bad_inf)):
            with pytest.raises(evplp.EvplpError) as e:
                c.update_mesh(*args)
            assert e.value.status == evplp.ERR_INVALID
        assert L.evplp_update_mesh(c._h, m0, None, good.shape[0]) == evplp.ERR_INVALID
        # nothing was marked dirty by a refused update: the passes still run, and a refit has nothing to do
        c.refit_accel()
        assert c.refit_info() == {"refits": 0, "levels": 0, "last_refit_ms": 0.0}
        c.primary(JITTER, clear_light=True)
        # a valid update: every pass is refused until the refit
        apply(c, mo)
        cam = c.camera()
        fp = evplp.frame_params(camera_pos=list(cam.origin), num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
        for call in (lambda: c.primary(JITTER, clear_light=True), lambda: c.trace_light_paths(7), lambda: c.gather_vpl(fp), lambda: c.gather_lvc(fp),
                     lambda: c.splat_photons(fp, clear=True), lambda: c.path_trace(list(cam.origin), 5, 3)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value) and "evplp_build_accel" in str(e.value)
        c.refit_accel()
        same(render(evplp, c), fresh_frames["a"], "after the refusals")
        assert c.refit_info()["refits"] == 1
        c.refit_accel()                                                       # nothing dirty: nothing happens
        assert c.refit_info()["refits"] == 1
        # a dirty context may also be rebuilt
        apply(c, {m: room.meshes[m]["verts"] for m in mo})
        c.build_accel()
        same(render(evplp, c), before, "rebuilt from the original vertices")
        # a refit of unmoved vertices changes no byte
        apply(c, {m: room.meshes[m]["verts"] for m in mo})
        c.refit_accel()
        same(render(evplp, c), before, "refit of unmoved vertices")


# ---- 7
def group_frame_params(evplp, sd, total, seed):
    return evplp.frame_params(camera_pos=sd.cam_origin, mis_mode=1, pdf_mc=0.4, clamping_value=1.0 / total, photon_radius=0.3, num_light_paths=NPATHS,
                              num_vpl_light_paths=NPATHS, photons_per_path=P, do_accumulate=1, rng_seed=seed, jitter=JITTER)


def test_group_strips(evplp, room, fresh_frames):
    mo = motion_a(room)
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        room.upload(c)
        apply(c, mo); c.refit_accel()
        _, total, _ = c.scene_metrics()
        fp = group_frame_params(evplp, room, total, 7)
        c.clear_accumulators()
        c.primary(JITTER, clear_light=True); c.trace_light_paths(7); c.gather_vpl(fp); c.splat_photons(fp)
        want = c.resolve(1.0, 1.0, 1.0)[:H]
    assert want.max() > 0
    with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True) as g:
        for r in range(2):
            room.upload(g.rank(r))
        with pytest.raises(evplp.EvplpError) as e:                            # refused on the caller's thread: the group stays usable
            g.update_mesh(box_meshes(0)[0], mo[box_meshes(0)[0]][:-1])
        assert e.value.status == evplp.ERR_INVALID
        for m, v in mo.items():
            g.update_mesh(m, v)
        with pytest.raises(evplp.EvplpError) as e:                            # dirty: a pass is refused, and the group stays usable
            g.primary(JITTER, 1)
        assert e.value.status == evplp.ERR_INVALID and "evplp_group_refit_accel" in str(e.value)
        g.refit_accel()
        assert all(g.rank(r).refit_info()["refits"] == 1 for r in range(2))
        g.clear_accumulators()
        g.primary(JITTER, 1); g.trace_light_paths(7); g.gather(fp, 0); g.splat_photons(fp)
        got = g.resolve(1.0, 1.0, 1.0)
    assert got.tobytes() == want.tobytes()


def test_group_iterations(evplp, room):
    mo = motion_a(room)
    js = [JITTER, (-0.003, 0.002)]
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:
        room.upload(c)
        apply(c, mo); c.refit_accel()
        _, total, _ = c.scene_metrics()
        c.clear_accumulators()
        for i in range(2):
            fp = group_frame_params(evplp, room, total, 7 + i)
            c.primary(js[i]); c.trace_light_paths(7 + i); c.gather_vpl(fp); c.splat_photons(fp)
        want = c.resolve(0.5, 0.5, 1.0)[:H].astype(np.float64)
    with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True, partition="iterations") as g:
        for r in range(2):
            room.upload(g.rank(r))
        for m, v in mo.items():
            g.update_mesh(m, v)
        g.refit_accel()
        g.clear_accumulators()
        for i in range(2):
            g.select_rank(i)
            fp = group_frame_params(evplp, room, total, 7 + i)
            g.primary(js[i]); g.trace_light_paths(7 + i); g.gather(fp, 0); g.splat_photons(fp)
        got = g.resolve(0.5, 0.5, 1.0)
    assert want.max() > 0
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-6
