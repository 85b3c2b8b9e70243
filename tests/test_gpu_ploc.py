"""The device PLOC builder (EVPLP_BVH_PLOC_GPU = 4): it runs and says so, its frames equal the SAH tree's bit for bit, its tree equals the host
twin's (evplp_ploc_tree) at the window's edges and in the pairing phase, and everything downstream of a build serves it as it serves the other
builders -- the quality figure, the refit, the refit policy through rebuild_builder = -1, groups.  Frames, motions and the figure's check are
test_gpu_bvh.py's and test_gpu_accel_quality.py's, restated or imported."""
import os

import numpy as np
import pytest

import scenes
from test_gpu_accel_quality import apply, box_meshes, check, doubles, group_frame, moved_room, same, translate
from test_gpu_accel_quality import render as full_frame
from test_ploc_host import copies, nested, subtree_info

pytestmark = pytest.mark.gpu

W, H = 96, 64
NPATHS, P = 64, 4
SAH, LBVH_GPU, PLOC = 1, 3, 4
MAX_DEPTH = 64
F = np.float32
# the developer override that forces one builder on every context (a whole-suite run per builder): the SAH and device-LBVH contexts these tests
# compare against are then PLOC trees too, so what is asserted ABOUT them (which builder ran, a cost to beat) has no subject
FORCED = os.environ.get("EVPLP_BVH_BUILDER")


@pytest.fixture(scope="module")
def room():
    return scenes.box_room(seed=11, n_boxes=7, tess=3, aspect=W / H)


def context(evplp, builder=PLOC, **kw):
    return evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=builder, deterministic=True, **kw)


def builder_of(evplp, c):
    return evplp.lib().evplp_accel_builder(c._h)


# ---- builder and frame (test_every_builder_gives_the_same_frame's comparison)
def render(evplp, room, builder, mis_mode=1):
    with context(evplp, builder) as c:
        room.upload(c)
        info = c.accel_info()
        used = builder_of(evplp, c)
        c.clear_accumulators()
        c.primary((0.002, -0.001), clear_light=True)
        c.trace_light_paths(7)
        cam = c.camera()
        _, total, _ = c.scene_metrics()
        fp = evplp.frame_params(camera_pos=list(cam.origin), mis_mode=mis_mode, pdf_mc=0.4, clamping_value=1.0 / total, photon_radius=0.3,
                                num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P, rng_seed=7)
        c.gather_vpl(fp)
        c.splat_photons(fp, clear=True)
        return {
            "gbuf": [c.download(b)[:H].copy() for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_LIGHT)],
            "records": c.download(evplp.BUF_RECORDS).copy(),
            "vpl": c.download(evplp.BUF_VPL_ACCUM)[:H].copy(),
            "photon": c.download(evplp.BUF_PHOTON_ACCUM)[:H].copy(),
            "rays": c.pass_stats(evplp.PASS_GATHER_VPL)["rays"],
            "info": info, "builder": used,
        }


def test_the_builder_runs_and_gives_the_sah_trees_frame(room, evplp):
    r, ref = render(evplp, room, PLOC), render(evplp, room, SAH)
    assert r["builder"] == 4 and r["info"]["builder"] == "ploc" and (FORCED or ref["builder"] == 1)
    assert ref["rays"] > 0 and np.isfinite(ref["vpl"]).all() and ref["vpl"][..., :3].max() > 0 and ref["photon"][..., :3].max() > 0
    assert r["info"]["nodes"] >= 1 and r["info"]["leaves"] >= 1 and 1 <= r["info"]["depth"] < 62, r["info"]
    assert r["info"]["stack4_entries"] > 0, "a parent's node index is below its children's: the four-wide stack bound is the computed one"
    for a, b in zip(r["gbuf"], ref["gbuf"]):
        assert np.array_equal(a, b), "G-buffer differs from the SAH tree's"
    assert r["records"].tobytes() == ref["records"].tobytes(), "light-path records differ"
    assert r["rays"] == ref["rays"], (r["rays"], ref["rays"])
    assert r["vpl"].tobytes() == ref["vpl"].tobytes(), "VPL gather differs"
    assert r["photon"].tobytes() == ref["photon"].tobytes(), "photon splat differs"


# ---- tiny scenes (test_tiny_scenes_build_on_the_device's)
def tiny_scene(ntri):
    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F)
    light = (quad + np.array([0, 2.0, 0], F), np.array([[0, 1, 2], [0, 2, 3]][:2 if ntri else 1], np.int32))
    fl = []
    for k in range(ntri):
        x = -1.0 + 2.0 * k / ntri
        fl.append([[x, -1.0, -1.0], [x + 2.0 / ntri, -1.0, -1.0], [x + 1.0 / ntri, -1.0, 1.0]])
    fl.append([[0, -1, 0], [0, -1, 0], [0, -1, 0]])                          # one degenerate
    fl = np.array(fl, F).reshape(-1, 3)
    return light, (fl, np.arange(len(fl), dtype=np.int32).reshape(-1, 3))


def build_meshes(evplp, c, meshes):
    """meshes[0] is the light; returns the triangle soup in mesh order (9 floats per triangle)"""
    m = c.add_material((0.6, 0.6, 0.6), (0.0, 0.0, 0.0), 1.0)
    ids = [c.add_mesh(v, i, m) for v, i in meshes]
    c.set_arealight(ids[0], (10.0, 10.0, 10.0, 0.0))
    c.set_camera((0.0, 0.5, 3.5), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 0.9, 1.0)
    c.build_accel()
    return np.concatenate([v[i].reshape(-1, 9) for v, i in meshes]).astype(F)


@pytest.mark.parametrize("ntri", [0, 1, 2, 4, 9])
def test_tiny_scenes(evplp, ntri):
    results = {}
    for name, b in (("sah", SAH), ("ploc", PLOC)):
        with evplp.Context(32, 32, 16, 16, 4, bvh_builder=b) as c:
            build_meshes(evplp, c, tiny_scene(ntri))
            assert FORCED or builder_of(evplp, c) == b
            c.primary((0.0, 0.0), clear_light=True)
            c.trace_light_paths(1)
            results[name] = (c.download(evplp.BUF_GBUF_POSITION).tobytes(), c.download(evplp.BUF_GBUF_NORMAL).tobytes(), c.download(evplp.BUF_RECORDS).tobytes())
    assert results["ploc"] == results["sah"]
    assert np.frombuffer(results["sah"][0], F).any() or ntri == 0, "the floor should be visible"


# ---- topology
def device_nested(evplp, c):
    """the tree on the device as nested (left, right) tuples with a sorted tuple of original triangles per leaf block"""
    nodes, ti = c.debug_accel(0), c.debug_accel(3)

    def of(r):
        r = int(r)
        if r >= 0:
            return (of(nodes["c0"][r]), of(nodes["c1"][r]))
        slot, cnt = ~r & ~3, (~r & 3) + 1
        return tuple(sorted(int(t) for t in ti[slot:slot + cnt]))
    if int(nodes["c1"][0]) == evplp.NO_CHILD:                                 # at most 4 triangles: a root with the block as its only child
        return of(nodes["c0"][0]) if int(nodes["c0"][0]) != evplp.NO_CHILD else ()
    return of(0)


SETTINGS = [("EVPLP_PLOC_RADIUS", 1), ("EVPLP_PLOC_RADIUS", 2), ("EVPLP_PLOC_RADIUS", 16), ("EVPLP_PLOC_ITERATIONS", 0), ("EVPLP_PLOC_ITERATIONS", 3)]


def twin(evplp, verts9, var, value):
    kw = dict(radius=value) if var == "EVPLP_PLOC_RADIUS" else dict(search_iterations=value)
    order, children, it = evplp.ploc_tree(verts9, **kw)
    hk = subtree_info(children, len(order))[2]
    return nested(order, children), it, (int(hk[0]) if len(hk) else 0) + 2


@pytest.mark.parametrize("var, value", SETTINGS)
def test_the_device_tree_is_the_twins(evplp, room, monkeypatch, var, value):
    monkeypatch.setenv(var, str(value))                                       # (read once by evplp_create; restored when the test ends)
    want, it, depth = twin(evplp, room.triangle_soup()[0], var, value)
    assert depth <= MAX_DEPTH - 2
    with context(evplp) as c:
        room.upload(c)
        assert builder_of(evplp, c) == 4 and c.accel_info()["depth"] == depth
        assert device_nested(evplp, c) == want, f"{var}={value}: the device tree differs from evplp_ploc_tree's ({it} iterations)"


@pytest.mark.parametrize("var, value", SETTINGS)
def test_the_device_tree_is_the_twins_where_everything_ties(evplp, monkeypatch, var, value):
    """64 copies of one triangle plus the light.  Every distance among the copies ties, so every search iteration merges position 0 and 1 of
    them and nothing else: under the search the tree is a chain whose 61 kept levels (+ 2) pass the walks' stack, and the builder does what
    evplp_build_accel documents for a tree that deep -- the host SAH tree, reported as builder 1.  The twin says which case a setting is
    (depth from its tree, by the builder's own rule); with 0 and 3 search iterations the pairing keeps the tree shallow and the two are equal."""
    monkeypatch.setenv(var, str(value))
    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], F) + np.array([0, 2.0, 0], F)
    tri = copies(64).reshape(-1, 3)
    with evplp.Context(32, 32, 16, 16, 4, bvh_builder=PLOC) as c:
        soup = build_meshes(evplp, c, [(quad, np.array([[0, 1, 2], [0, 2, 3]], np.int32)), (tri, np.arange(192, dtype=np.int32).reshape(-1, 3))])
        want, it, depth = twin(evplp, soup, var, value)
        assert (depth <= MAX_DEPTH - 2) == (var == "EVPLP_PLOC_ITERATIONS"), (var, value, depth)
        if depth > MAX_DEPTH - 2:
            assert builder_of(evplp, c) == 1, f"a PLOC tree of depth {depth} is replaced by the host SAH tree"
            assert c.accel_info()["depth"] <= MAX_DEPTH - 2
        else:
            assert builder_of(evplp, c) == 4 and c.accel_info()["depth"] == depth
            assert device_nested(evplp, c) == want, f"{var}={value}: the device tree differs from evplp_ploc_tree's ({it} iterations)"
        c.primary((0.0, 0.0), clear_light=True)                               # and the tree serves a walk
        assert np.isfinite(c.download(evplp.BUF_GBUF_POSITION)).all()


def test_overrides_out_of_range_are_refused(evplp, monkeypatch):
    for var, bad in (("EVPLP_PLOC_RADIUS", "0"), ("EVPLP_PLOC_RADIUS", "33"), ("EVPLP_PLOC_RADIUS", "x"), ("EVPLP_PLOC_ITERATIONS", "-1"), ("EVPLP_PLOC_ITERATIONS", "129")):
        monkeypatch.setenv(var, bad)
        with pytest.raises(evplp.EvplpError) as e:
            context(evplp)
        assert e.value.status == evplp.ERR_INVALID and var in str(e.value)
        monkeypatch.delenv(var)


# ---- the quality figure
def test_the_quality_figure_and_the_cost_against_the_device_lbvh(evplp, room):
    with context(evplp) as c:
        room.upload(c)
        q = check(evplp, c, "ploc, built")                                    # the kernel equals evplp_accel_cost on the downloaded nodes bit for bit
    if FORCED:
        return
    with context(evplp, LBVH_GPU) as c:
        room.upload(c)
        ql = c.accel_quality()
    assert q["cost"] < ql["cost"], f"PLOC cost {q['cost']:.4f}, device LBVH cost {ql['cost']:.4f}"
    print(f"PLOC cost {q['cost']:.4f}, device LBVH cost {ql['cost']:.4f}, ratio {q['cost'] / ql['cost']:.4f}")


# ---- refit and policy
def two_boxes(room):
    mo = translate(room, box_meshes(1), (0.3, -0.25, 0.0))
    mo.update(translate(room, box_meshes(4), (-0.4, 0.2, 0.0)))
    return mo


@pytest.fixture(scope="module")
def fresh_moved(evplp, room):
    """a fresh PLOC build of the room with two boxes moved: frame, nodes, figure"""
    with context(evplp) as c:
        moved_room(room, two_boxes(room)).upload(c)
        assert builder_of(evplp, c) == 4
        out = {"frame": full_frame(evplp, c), "nodes": c.debug_accel(0).tobytes(), "q": c.accel_quality()}
    assert all(np.frombuffer(out["frame"][k], F).max() > 0 for k in ("vpl", "lvc", "photon"))
    return out


def test_a_refitted_ploc_tree_gives_the_fresh_builds_frame(evplp, room, fresh_moved):
    with context(evplp) as c:
        room.upload(c)
        before = c.debug_accel(0).tobytes()
        apply(c, two_boxes(room)); c.refit_accel()
        assert builder_of(evplp, c) == 4 and c.debug_accel(0).tobytes() != before
        same(full_frame(evplp, c), fresh_moved["frame"], "the refitted PLOC tree")
        check(evplp, c, "ploc, refitted")


def test_the_policy_rebuilds_with_the_contexts_own_builder(evplp, room, fresh_moved):
    with context(evplp) as c:
        room.upload(c)
        q0 = c.accel_quality()
        apply(c, two_boxes(room)); c.refit_accel()
        r = c.accel_quality()["cost"] / q0["cost"]
    print(f"refitted / built: {r:.6f}")
    with context(evplp) as c:
        room.upload(c)
        with pytest.raises(evplp.EvplpError):                                 # (4 as rebuild_builder stays refused: -1 is the way)
            c.set_refit_policy(0.99 * r, PLOC)
        c.set_refit_policy(0.99 * r, -1)
        apply(c, two_boxes(room)); c.refit_accel()
        q = c.accel_quality()
        assert q["policy_rebuilds"] == 1 and q["last_action"] == 2 and q["refits_since_build"] == 0
        assert builder_of(evplp, c) == 4
        assert c.debug_accel(0).tobytes() == fresh_moved["nodes"] and doubles(q) == doubles(fresh_moved["q"])
        same(full_frame(evplp, c), fresh_moved["frame"], "the policy's PLOC rebuild")


# ---- groups
def test_a_two_rank_group_gives_the_single_contexts_frame(evplp, room):
    with context(evplp) as c:
        room.upload(c)
        total = c.scene_metrics()[1]
        want = group_frame(evplp, c, room, total)
    with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True, strip_rows=8, bvh_builder=PLOC) as g:
        for r in range(2):
            room.upload(g.rank(r))
            assert builder_of(evplp, g.rank(r)) == 4
        assert g.rank(0).debug_accel(0).tobytes() == g.rank(1).debug_accel(0).tobytes()
        got = group_frame(evplp, g, room, total)
    assert np.frombuffer(want, F).max() > 0
    assert got == want, "two ranks over PLOC trees: the frame differs from the single context's"
