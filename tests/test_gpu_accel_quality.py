"""The tree's SAH cost on the device (evplp_accel_quality) and the refit policy (evplp_set_refit_policy).  The kernel's five doubles are held
to the host function evplp_accel_cost on the downloaded node bytes bit for bit, and to math.fsum of the same terms within the bound derived in
test_accel_quality_host.py; the call only measures; a motion built to age the tree shows in the figure; and the policy rebuilds exactly when
the figure crosses its ratio -- on one context and on every rank of a group.  Helpers and motions are test_gpu_refit.py's, restated."""
import copy
import math

import numpy as np
import pytest

import scenes
from test_accel_quality_host import KEYS, fsum_cost, within_the_bound

pytestmark = pytest.mark.gpu

W, H = 96, 64
NPATHS, P = 64, 4
BUILDERS = {"lbvh": 0, "sah": 1, "sbvh": 2, "gpu": 3}
JITTER = (0.002, -0.001)
F = np.float32
COUNTERS = ("built_cost", "refits_since_build", "policy_rebuilds", "last_action")


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
    return mo


def motion_b(room, room_a):
    """on top of A: box 0 back to where it was, box 5 moved"""
    mo = {m: room.meshes[m]["verts"].copy() for m in box_meshes(0)}
    mo.update(translate(room_a, box_meshes(5), (-0.3, 0.25, 0.0)))
    return mo


def box_centre(room, b):
    allv = np.concatenate([room.meshes[m]["verts"] for m in box_meshes(b)])
    return (F(0.5) * (allv.min(0) + allv.max(0))).astype(F)


# six places far from each other (x, y, under the ceiling?), clear of the camera at (9.2, 0.9, 3.2) and of the light above the middle of the room
PLACES = [(1.2, 1.2, False), (8.8, 6.8, False), (1.2, 6.8, True), (5.0, 1.2, True), (5.0, 6.8, False), (8.8, 4.0, True)]


def motion_scatter(room):
    """The motion built to age a tree: face k of every box goes, rigidly, to place k -- three of the six on the floor, three hanging under the
    ceiling, all near the walls of the 10 x 8 x 5 room (a small offset per box keeps the faces of different boxes apart).  A builder puts a
    box's 108 triangles under one subtree.  After the refit every node of that subtree above a single face -- five per box, and every leaf or
    node that held triangles of two faces along a shared edge -- spans the distance between places: the node of all six faces is the whole room
    (area 340, the root's own), the nodes of two or three faces are a large part of it, where the built tree had a box of a few square
    metres.  A fresh build of the moved scene clusters by place again, and since the triangles keep their size its cost stays about what it
    was (the built tree's inner_area is 19 root areas, its cost 399); the refitted tree pays 15 per root area for every root area those
    nodes grow by -- five nodes of a third of the room to all of it for each of seven boxes is some twenty root areas, about 300 on top of
    400, and the nodes that mixed two faces along an edge add to it (seen on the device: 2.5 times the fresh build's cost)."""
    mo = {}
    for b in range(7):
        allv = np.concatenate([room.meshes[m]["verts"] for m in box_meshes(b)])
        ctr, top = box_centre(room, b), allv[:, 2].max()
        for k, m in enumerate(box_meshes(b)):
            x, y, up = PLACES[k]
            d = np.array([x + 0.07 * b - ctr[0], y - 0.07 * b - ctr[1], (4.6 - top) if up else 0.0], F)
            mo[m] = (room.meshes[m]["verts"] + d).astype(F)
    return mo


def apply(c, motion):
    for m, v in motion.items():
        c.update_mesh(m, v)


def render(evplp, c):
    """test_gpu_refit.py's frame: the G-buffer, light paths, VPL and LVC gathers with their ray counts, a path trace on top, the photon splat"""
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


def context(evplp, builder="sah"):
    return evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True)


def doubles(q):
    return {k: q[k] for k in KEYS}


def check(evplp, c, what):
    """the kernel against the host function on the node bytes as they are (bit for bit) and against fsum (the derived bound); returns the figures"""
    q = c.accel_quality()
    nodes = c.debug_accel(0)
    host = evplp.accel_cost(nodes)
    assert doubles(q) == doubles(host), f"{what}: the kernel's doubles differ from evplp_accel_cost's"
    assert q["reached_nodes"] == host["reached_nodes"] <= len(nodes)
    reached = nodes[evplp.refit_levels(nodes, level_capacity=len(nodes))[1]]
    assert q["leaf_refs"] == sum(int(((reached[s] < 0) & (reached[s] != evplp.NO_CHILD)).sum()) for s in ("c0", "c1"))
    print(f"{what}: reached {q['reached_nodes']} cost {q['cost']:.6f} root {q['root_area']:.6f} inner {q['inner_area']:.6f} pair {q['leaf_pair_area']:.6f} tri {q['leaf_tri_area']:.6f}")
    within_the_bound(dict(doubles(q), reached_nodes=q["reached_nodes"]), fsum_cost(evplp, nodes))
    assert q["cost"] > 15.0 and q["root_area"] > 0 and q["leaf_tri_area"] >= q["leaf_pair_area"] > 0
    return q


@pytest.fixture(scope="module")
def scattered(room):
    return moved_room(room, motion_scatter(room))


@pytest.fixture(scope="module")
def fresh_scattered(evplp, scattered):
    """the reference of the ageing and policy tests, made once: a fresh SAH build of the scattered room -- frame, node bytes, figures"""
    with context(evplp) as c:
        scattered.upload(c)
        out = {"frame": render(evplp, c), "nodes": c.debug_accel(0).tobytes(), "q": c.accel_quality()}
    assert all(np.frombuffer(out["frame"][k], F).max() > 0 for k in ("vpl", "lvc", "photon")), "the scattered room renders black"
    return out


def same(got, want, what):
    for k, v in want.items():
        assert got[k] == v, f"{what}: {k} differs from the fresh build's"


# ---- 1
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_the_kernel_equals_the_host_function(evplp, room, builder):
    room_a = moved_room(room, motion_a(room))
    with context(evplp, builder) as c:
        room.upload(c)
        q0 = check(evplp, c, f"{builder}, built")
        assert q0["built_cost"] == q0["cost"] and q0["refits_since_build"] == 0
        apply(c, motion_a(room)); c.refit_accel()
        qa = check(evplp, c, f"{builder}, motion A")
        apply(c, motion_b(room, room_a)); c.refit_accel()
        qb = check(evplp, c, f"{builder}, motion B")
        assert qa["cost"] != q0["cost"] and qb["cost"] != qa["cost"], "the motions do not show in the figure"
        assert qb["built_cost"] == q0["cost"] and qb["refits_since_build"] == 2 and qb["reached_nodes"] == q0["reached_nodes"]


def test_more_than_one_chunk_and_a_chunk_that_is_mostly_padding(evplp, room):
    """at least one of the four builders' trees of the room fills more than one 256-entry chunk; the smallest room is one ragged chunk"""
    reached = {}
    for builder in BUILDERS:
        with context(evplp, builder) as c:
            room.upload(c)
            reached[builder] = c.accel_quality()["reached_nodes"]
    print(reached)
    assert max(reached.values()) > 256, reached
    small = scenes.box_room(seed=11, n_boxes=0, tess=1, aspect=W / H)
    for builder in ("sah", "gpu"):
        with context(evplp, builder) as c:
            small.upload(c)
            q = check(evplp, c, f"{builder}, the empty room")
            assert q["reached_nodes"] < 128


# ---- 2
def test_it_only_measures(evplp, room):
    with context(evplp) as c:
        room.upload(c)
        apply(c, motion_a(room)); c.refit_accel()
        before = (c.debug_accel(0).tobytes(), c.debug_accel(4).tobytes(), render(evplp, c), c.refit_info()["refits"])
        q1 = c.accel_quality()
        q2 = c.accel_quality()
        assert q1 == q2
        after = (c.debug_accel(0).tobytes(), c.debug_accel(4).tobytes(), render(evplp, c), c.refit_info()["refits"])
        assert before[0] == after[0] and before[1] == after[1] and before[3] == after[3]
        same(after[2], before[2], "after two evplp_accel_quality calls")
        assert c.accel_quality() == q1


# ---- 3
def test_refusals(evplp, room):
    with context(evplp) as c:
        with pytest.raises(evplp.EvplpError) as e:                            # no accel built
            c.accel_quality()
        assert e.value.status == evplp.ERR_INVALID
        c.set_refit_policy(0.0)                                               # (nothing to measure, nothing dirty: accepted)
        for bad in ((-1.0, -1), (float("nan"), -1), (float("inf"), -1), (1.5, 4), (1.5, -2)):
            with pytest.raises(evplp.EvplpError) as e:
                c.set_refit_policy(*bad)
            assert e.value.status == evplp.ERR_INVALID
        room.upload(c)
        assert evplp.lib().evplp_accel_quality(c._h, None) == evplp.ERR_INVALID
        apply(c, motion_a(room))
        for call in (c.accel_quality, lambda: c.set_refit_policy(1.5), lambda: c.set_refit_policy(0.0)):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value) and "evplp_build_accel" in str(e.value)
        c.refit_accel()
        q = c.accel_quality()
        assert q["last_action"] == 0 and q["policy_rebuilds"] == 0 and q["refits_since_build"] == 1


# ---- 4
def test_a_degenerate_triangle_still_counts(evplp, room):
    with context(evplp) as c:
        room.upload(c)
        nodes, ti = c.debug_accel(0), c.debug_accel(3)
        # a leaf of two triangles or more (this room's SAH leaves hold the two triangles of a quad), and the mesh and vertices of its first one
        refs = np.concatenate([nodes["c0"], nodes["c1"]])
        first = np.cumsum([0] + [len(m["idx"]) for m in room.meshes])
        mesh_of = lambda t: int(np.searchsorted(first, t, side="right") - 1)
        full = [int(r) for r in refs if r < 0 and r != evplp.NO_CHILD and (~int(r) & 3) >= 1 and mesh_of(int(ti[4 * (~int(r) >> 2)])) != room.light_mesh]
        assert full, "no leaf of two triangles"
        tri = int(ti[4 * (~full[0] >> 2)])
        mesh = mesh_of(tri)
        idx = np.asarray(room.meshes[mesh]["idx"]).reshape(-1, 3)[tri - first[mesh]]
        q0 = check(evplp, c, "before the collapse")
        v = room.meshes[mesh]["verts"].copy()
        # the triangle becomes a sliver of no area ALONG one of its own edges (its third vertex goes to the middle of the other two), so the leaf's
        # box can only shrink; its neighbours in the mesh share the moved vertex and change shape, so the comparison below is of counts
        v[idx[2]] = (F(0.5) * (v[idx[0]] + v[idx[1]])).astype(F)
        c.update_mesh(mesh, v); c.refit_accel()
        q1 = check(evplp, c, "after the collapse")                            # kernel and host function still agree
        nodes1 = c.debug_accel(0)
        for s in ("c0", "c1"):
            assert np.array_equal(nodes1[s], nodes[s])                        # the reference keeps its count ...
        # ... and the leaf is still charged for every slot: leaf_tri_area is the sum over the references' counts
        tri_sum = math.fsum(8.0 * (float(n["hal"][0, s]) * float(n["hal"][1, s]) + float(n["hal"][1, s]) * float(n["hal"][2, s]) + float(n["hal"][2, s]) * float(n["hal"][0, s]))
                            * ((~int(r) & 3) + 1) for n in nodes1 for s, r in enumerate((n["c0"], n["c1"])) if r < 0 and r != evplp.NO_CHILD and n["hal"][:, s].min() >= 0)
        tol = q1["reached_nodes"] * 2.0 ** -52 * tri_sum
        assert abs(q1["leaf_tri_area"] - tri_sum) <= tol
        # (charged for the live ones alone, the sum would be lower by the leaf's own area, far more than the bound)
        own = [8.0 * (float(n["hal"][0, s]) * float(n["hal"][1, s]) + float(n["hal"][1, s]) * float(n["hal"][2, s]) + float(n["hal"][2, s]) * float(n["hal"][0, s]))
               for n in nodes1 for s, r in enumerate((n["c0"], n["c1"])) if r == full[0]]
        assert len(own) == 1 and own[0] > 1e6 * tol
        assert q1["leaf_refs"] == q0["leaf_refs"] and q1["reached_nodes"] == q0["reached_nodes"]


# ---- 5
def test_ageing_shows(evplp, room, scattered, fresh_scattered):
    fq = fresh_scattered["q"]
    with context(evplp) as c:
        room.upload(c)
        q0 = check(evplp, c, "built")
        apply(c, motion_scatter(room)); c.refit_accel()
        q = check(evplp, c, "scattered, refitted")
        print(f"refitted / fresh build of the scattered room: {q['cost'] / fq['cost']:.4f}; refitted / built: {q['cost'] / q0['cost']:.4f}; fresh / built: {fq['cost'] / q0['cost']:.4f}")
        assert q["cost"] > fq["cost"], "the refitted tree of the scattered room should cost more than a fresh build of it"
        assert q["inner_area"] > fq["inner_area"]
        same(render(evplp, c), fresh_scattered["frame"], "the refitted tree")
        c.build_accel()
        assert c.debug_accel(0).tobytes() == fresh_scattered["nodes"]
        qr = c.accel_quality()
        assert doubles(qr) == doubles(fq) and qr["built_cost"] == fq["cost"] and qr["refits_since_build"] == 0


# ---- 6
@pytest.fixture(scope="module")
def refit_scattered(evplp, room):
    """policy off: the plain refit's node bytes, and r = its cost over the built tree's.  The policy's counters (policy_rebuilds, last_action) and
    built_cost do not move; refits_since_build counts the refit, as it does with or without a policy"""
    with context(evplp) as c:
        room.upload(c)
        q0 = c.accel_quality()
        apply(c, motion_scatter(room)); c.refit_accel()
        q = c.accel_quality()
        assert {k: q[k] for k in COUNTERS} == {"built_cost": q0["cost"], "refits_since_build": 1, "policy_rebuilds": 0, "last_action": 0}
        return {"nodes": c.debug_accel(0).tobytes(), "r": q["cost"] / q0["cost"], "q": q}


def test_the_policy_rebuilds_below_the_ratio_and_keeps_above(evplp, room, refit_scattered, fresh_scattered):
    r = refit_scattered["r"]
    print(f"r = {r:.4f}")
    assert r > 1.02
    with context(evplp) as c:                                                 # 0.99 r: the refit rebuilds
        room.upload(c)
        c.set_refit_policy(0.99 * r)                                          # (measures built_cost there and then: the refit below has nothing else to compare with)
        built = refit_scattered["q"]["built_cost"]
        apply(c, motion_scatter(room)); c.refit_accel()
        q = c.accel_quality()
        assert q["last_action"] == 2 and q["policy_rebuilds"] == 1 and q["refits_since_build"] == 0
        assert doubles(q) == doubles(fresh_scattered["q"]) and q["built_cost"] == q["cost"] != built
        assert c.debug_accel(0).tobytes() == fresh_scattered["nodes"]
        same(render(evplp, c), fresh_scattered["frame"], "the policy's rebuild")
        assert c.refit_info()["refits"] == 1
        c.refit_accel()                                                       # nothing dirty: nothing happens
        assert c.accel_quality()["policy_rebuilds"] == 1
        c.build_accel()
        assert c.accel_quality()["last_action"] == 0
    with context(evplp) as c:                                                 # 1.01 r: it keeps the refit
        room.upload(c)
        c.set_refit_policy(1.01 * r)
        apply(c, motion_scatter(room)); c.refit_accel()
        q = c.accel_quality()
        assert q["last_action"] == 1 and q["policy_rebuilds"] == 0 and q["refits_since_build"] == 1
        assert doubles(q) == doubles(refit_scattered["q"])
        assert c.debug_accel(0).tobytes() == refit_scattered["nodes"]
        same(render(evplp, c), fresh_scattered["frame"], "the kept refit")


def test_the_policy_rebuilds_with_its_own_builder_and_leaves_the_accumulators(evplp, room, refit_scattered, fresh_scattered):
    with context(evplp) as c:
        room.upload(c)
        assert c.accel_info()["builder"] == "sah"
        c.set_refit_policy(0.99 * refit_scattered["r"], evplp.BVH_LBVH_GPU)
        render(evplp, c)
        acc = c.download(evplp.BUF_PHOTON_ACCUM).tobytes()
        assert np.frombuffer(acc, F).max() > 0
        apply(c, motion_scatter(room)); c.refit_accel()
        assert evplp.lib().evplp_accel_builder(c._h) == 3 and c.accel_info()["builder"] == "gpu"
        assert c.download(evplp.BUF_PHOTON_ACCUM).tobytes() == acc, "a policy rebuild leaves the accumulators alone"
        q = check(evplp, c, "rebuilt by the device LBVH")
        assert q["last_action"] == 2 and q["policy_rebuilds"] == 1 and q["built_cost"] == q["cost"]
        same(render(evplp, c), fresh_scattered["frame"], "the policy's device LBVH")
        c.set_refit_policy(0.0)                                               # off again: a refit is a refit
        apply(c, {m: room.meshes[m]["verts"] for m in motion_scatter(room)}); c.refit_accel()
        q2 = c.accel_quality()
        assert q2["last_action"] == 2 and q2["policy_rebuilds"] == 1 and q2["refits_since_build"] == 1 and q2["built_cost"] == q["cost"]


# ---- 7
def group_frame(evplp, g, room, total, ranks=(None,)):
    """one accumulated frame; ranks: the ranks of an iterations group that each render it (the resolve then averages equal images, exactly)"""
    fp = evplp.frame_params(camera_pos=room.cam_origin, mis_mode=1, pdf_mc=0.4, clamping_value=1.0 / total, photon_radius=0.3, num_light_paths=NPATHS,
                            num_vpl_light_paths=NPATHS, photons_per_path=P, do_accumulate=1, rng_seed=7, jitter=JITTER)
    g.clear_accumulators()
    for r in ranks:
        if r is not None:
            g.select_rank(r)
        if isinstance(g, evplp.Group):
            g.primary(JITTER, 1); g.trace_light_paths(7); g.gather(fp, 0); g.splat_photons(fp)
        else:
            g.primary(JITTER, clear_light=True); g.trace_light_paths(7); g.gather_vpl(fp); g.splat_photons(fp)
    return g.resolve(1.0 / len(ranks), 1.0 / len(ranks), 1.0)[:H].tobytes()


@pytest.fixture(scope="module")
def single_frame(evplp, scattered):
    with context(evplp) as c:
        scattered.upload(c)
        total = c.scene_metrics()[1]
        return total, group_frame(evplp, c, scattered, total)


@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("mode", ["round robin", "dealt", "iterations"])
def test_groups(evplp, room, refit_scattered, fresh_scattered, single_frame, mode, n):
    total, want = single_frame
    kw = dict(partition="iterations") if mode == "iterations" else dict(strip_rows=8)
    with evplp.Group(W, H, NPATHS, NPATHS, P, n, devices=[0] * n, deterministic=True, **kw) as g:
        for r in range(n):
            room.upload(g.rank(r))
        if mode == "dealt":
            g.calibrate(True); group_frame(evplp, g, room, g.rank(0).scene_metrics()[1]); g.rebalance()
        with pytest.raises(evplp.EvplpError) as e:                            # refused on the caller's thread: the group stays usable
            g.set_refit_policy(-1.0)
        assert e.value.status == evplp.ERR_INVALID
        assert evplp.lib().evplp_group_accel_quality(g._h, None) == evplp.ERR_INVALID
        q0 = g.accel_quality()
        assert q0["cost"] == refit_scattered["q"]["built_cost"]
        for m, v in motion_scatter(room).items():
            g.update_mesh(m, v)
        for call in (g.accel_quality, lambda: g.set_refit_policy(1.5)):       # dirty
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value)
        g.refit_accel()
        q = g.accel_quality()
        assert doubles(q) == doubles(refit_scattered["q"]) and q["last_action"] == 0 and q["refits_since_build"] == 1
        assert all(doubles(g.rank(r).accel_quality()) == doubles(q) for r in range(n))
        # a policy just under the ratio: back to the start it keeps the refit, scattered again every rank rebuilds
        g.set_refit_policy(0.99 * refit_scattered["r"])
        for m in motion_scatter(room):
            g.update_mesh(m, room.meshes[m]["verts"])
        g.refit_accel()
        q = g.accel_quality()
        assert q["last_action"] == 1 and q["policy_rebuilds"] == 0 and q["refits_since_build"] == 2 and q["built_cost"] == q0["cost"]
        for m, v in motion_scatter(room).items():
            g.update_mesh(m, v)
        g.refit_accel()
        q = g.accel_quality()
        assert q["last_action"] == 2 and q["policy_rebuilds"] == 1 and doubles(q) == doubles(fresh_scattered["q"])
        for r in range(n):
            qr = g.rank(r).accel_quality()
            assert qr["last_action"] == 2 and qr["policy_rebuilds"] == 1, r
            assert g.rank(r).debug_accel(0).tobytes() == fresh_scattered["nodes"], r
        got = group_frame(evplp, g, room, total, ranks=range(n) if mode == "iterations" else (None,))      # (n = 2, 4: x + x and the halving are exact)
    assert np.frombuffer(want, F).max() > 0
    assert got == want, f"{n} ranks, {mode}: the frame over the policy's rebuilt trees differs from the single context's"
