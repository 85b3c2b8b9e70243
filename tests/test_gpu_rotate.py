"""Tree rotations on the device (evplp_optimize_accel, evplp_set_refit_rotations) against the host twin evplp_rotate_tree reference for
reference, against what a plain refit of the rotated topology writes (byte for byte, and restated in numpy fp32), against a fresh build's
frame (bit for bit: visibility and closest hit are exact predicates over the triangles), and against the bounds the walks rely on.  The
aged tree is test_gpu_accel_quality.py's: every box face of the room moved to another place, then a plain refit.

What the twin takes on that fixture is asserted > 0 on the CPU before the device is asked; test 1's docstring has the counts per builder."""
import math

import numpy as np
import pytest

import rotate_restate as rr
import scenes
import walk_replay as wr
from test_accel_quality_host import KEYS, fsum_cost, within_the_bound
from test_gpu_accel_quality import F, H, JITTER, NPATHS, P, W, apply, fresh_scattered, motion_scatter, moved_room, render, room, same, scattered  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BUILDERS = {"sah": 1, "sbvh": 2, "lbvh": 0, "gpu": 3, "ploc": 4}
FRAME_KEYS = ("pos", "nrm", "dif", "phg", "light", "records", "vpl", "lvc", "lvc + pt", "photon")


def context(evplp, builder="sah"):
    return evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=BUILDERS[builder], deterministic=True)


def aged(evplp, room, builder):
    """the room under `builder`'s tree, scattered and plainly refitted"""
    c = context(evplp, builder)
    room.upload(c)
    apply(c, motion_scatter(room)); c.refit_accel()
    return c


def soup_of(sd):
    return sd.triangle_soup()[0].astype(F).reshape(-1, 9)


def refs(nodes):
    return np.stack([nodes["c0"], nodes["c1"]], axis=1)


# ---- 1
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("builder", list(BUILDERS))
def test_the_device_equals_the_twin(evplp, room, scattered, builder, passes):
    """Rotations per pass on the aged fixture (twin = device): sah [49, 13, 3] of 598 nodes, sbvh [116, 56, 30] of 611, lbvh and gpu
    [81, 43, 20] of 358, ploc [39, 7, 2] of 335 -- the figures this test prints; every builder's tree takes at least one in pass 1."""
    with aged(evplp, room, builder) as c:
        nodes0, ti = c.debug_accel(0), c.debug_accel(3)
        twin = evplp.rotate_tree(nodes0, ti, soup_of(scattered), passes)
        print(f"{builder}: {len(nodes0)} nodes, the twin's rotations per pass {twin['rotations']}, need {twin['need0']}")
        assert twin["rotations"][0] >= 1, "a fixture on which nothing rotates proves nothing"
        info0 = c.accel_info()
        n = c.optimize_accel(passes)
        nodes1, n4 = c.debug_accel(0), c.debug_accel(4)
        assert np.array_equal(refs(nodes1), twin["children"]), "the device's references differ from the twin's"
        assert n == sum(twin["rotations"])
        ri = c.rotation_info()
        assert ri["per_pass"][:passes] == twin["rotations"] and not any(ri["per_pass"][passes:]) and ri["last_call"] == n and ri["since_build"] == n and ri["refit_passes"] == 0
        info = c.accel_info()
        assert info["stack4_entries"] == twin["need0"] + 2 == wr.worst_case_entries(n4) + 2
        assert np.array_equal(n4["child"], wr.four_wide(nodes1)["child"])
        assert info["depth"] == info0["depth"] and wr.tree_levels(nodes1) <= wr.tree_levels(nodes0)
        assert np.array_equal(c.debug_accel(3), ti), "a leaf moved"
        assert c.accel_quality()["last_action"] == 3


# ---- 2
@pytest.mark.parametrize("builder", ["sah", "gpu", "ploc"])
def test_a_rotated_tree_is_what_a_refit_of_that_topology_writes(evplp, room, scattered, builder):
    mo = motion_scatter(room)
    with aged(evplp, room, builder) as c:
        assert c.optimize_accel(2) > 0
        nodes, n4, pad = c.debug_accel(0), c.debug_accel(4), c.debug_accel(5)
        apply(c, mo)                                                          # dirty with their own vertices; rotations off: the plain refit
        c.refit_accel()
        assert c.debug_accel(0).tobytes() == nodes.tobytes(), "a plain refit of the rotated topology writes other node bytes"
        assert c.debug_accel(4).tobytes() == n4.tobytes(), "... other four-wide node bytes"
        assert c.rotation_info()["last_call"] > 0 and c.refit_info()["refits"] == 2
        assert rr.restate_structure(evplp, nodes, n4, c.debug_accel(3), soup_of(scattered), pad) == len(nodes)


# ---- 3
def pt_two_samples(evplp, c):
    c.clear_accumulators()
    cam = c.camera()
    for seed in (5, 6):
        c.path_trace(list(cam.origin), seed, 3, accumulate=True)
    return c.download(evplp.BUF_VPL_ACCUM)[:H].tobytes()


@pytest.mark.parametrize("cuts", [None, "0"])
@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_frames_are_bit_identical(evplp, room, scattered, builder, cuts, monkeypatch):
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    if cuts is not None:
        monkeypatch.setenv("EVPLP_CUTS", cuts)                               # (read when the context is created: every walk starts at the root)
    with context(evplp, "sah") as c:                                          # a fresh SAH build of the moved scene
        scattered.upload(c)
        want, want_pt = render(evplp, c), pt_two_samples(evplp, c)
    assert all(np.frombuffer(want[k], F).max() > 0 for k in ("vpl", "lvc", "photon")) and np.frombuffer(want_pt, F).max() > 0
    with aged(evplp, room, builder) as c:
        assert c.optimize_accel(3) > 0
        got, got_pt = render(evplp, c), pt_two_samples(evplp, c)
    for k in FRAME_KEYS + ("vpl rays", "lvc rays"):
        assert got[k] == want[k], f"{builder}, EVPLP_CUTS={cuts}: {k} over the rotated tree differs from the fresh build's"
    assert got_pt == want_pt, f"{builder}, EVPLP_CUTS={cuts}: the path tracer's accumulator after two samples differs"


# ---- 4
def test_the_cost_falls_and_only_the_tree_changed(evplp, room, scattered):
    with aged(evplp, room, "sah") as c:
        _, total, _ = c.scene_metrics()
        cam = c.camera()
        c.clear_accumulators()
        c.noise_track(True)
        for i in range(2):
            fp = evplp.frame_params(camera_pos=list(cam.origin), mis_mode=1, pdf_mc=0.4, clamping_value=1.0 / total, photon_radius=0.3, num_light_paths=NPATHS,
                                    num_vpl_light_paths=NPATHS, photons_per_path=P, do_accumulate=1, rng_seed=7 + i, jitter=JITTER)
            c.primary(JITTER, clear_light=(i == 0)); c.trace_light_paths(7 + i); c.gather_vpl(fp); c.splat_photons(fp)
            c.noise_fold(1)
        planes = lambda: [c.download(b).tobytes() for b in (evplp.BUF_VPL_ACCUM, evplp.BUF_PHOTON_ACCUM, evplp.BUF_LIGHT)] + [c.noise_variance(0.5).tobytes(), c.noise_estimate(0.5)]
        before, q0 = planes(), c.accel_quality()
        n = c.optimize_accel(2)
        q1 = c.accel_quality()
        host = evplp.accel_cost(c.debug_accel(0))                             # on the CPU: the rotated bytes cost what the device says, and less than before
        print(f"sah, scattered: refitted cost {q0['cost']:.4f}, after {n} rotations in 2 passes {q1['cost']:.4f} (built {q1['built_cost']:.4f}); inner area {q0['inner_area']:.2f} -> {q1['inner_area']:.2f}")
        # (the device sums in the PLAN's order, the host function in evplp_refit_levels' order of the rotated bytes: the same terms, other
        # roundings -- both lie within the bound test_accel_quality_host.py derives around the exact sum)
        assert n > 0
        exact = fsum_cost(evplp, c.debug_accel(0))
        within_the_bound({k: q1[k] for k in KEYS + ("reached_nodes",)}, exact)
        within_the_bound(host, exact)
        assert (q1["reached_nodes"], q1["leaf_refs"]) == (q0["reached_nodes"], q0["leaf_refs"]) and host["reached_nodes"] == q0["reached_nodes"]
        assert q1["cost"] < q0["cost"] and q1["inner_area"] < q0["inner_area"] and q1["root_area"] == q0["root_area"]
        # the leaves' terms are the same positive numbers, met in another order (a leaf hangs in another node's slot): each sum of leaf_refs
        # terms is within (leaf_refs - 1) 2^-53 of the exact one to first order, so the two are within leaf_refs 2^-52 of each other
        for k in ("leaf_pair_area", "leaf_tri_area"):
            assert abs(q1[k] - q0[k]) <= q0["leaf_refs"] * 2.0 ** -52 * q0[k], f"{k}: a leaf's box changed"
        assert (q1["built_cost"], q1["refits_since_build"], q1["policy_rebuilds"]) == (q0["built_cost"], q0["refits_since_build"], 0) and q1["last_action"] == 3
        assert planes() == before, "accumulators or noise moments moved"
        assert c.refit_info()["refits"] == 1


# ---- 5
def test_inside_the_refit(evplp, room, scattered):
    """The first pass of a rotating refit sees what a plain refit followed by one rotating pass sees -- the moved triangles and the built
    topology -- so evplp_set_refit_rotations(2) + one refit writes the bytes of a plain refit + evplp_optimize_accel(2)."""
    mo = motion_scatter(room)
    with context(evplp) as c:
        room.upload(c)
        c.accel_quality()                                                     # (built_cost: the first measurement since the build)
        apply(c, mo); c.refit_accel()
        q_plain = c.accel_quality()
        n = c.optimize_accel(2)
        want = (c.debug_accel(0).tobytes(), c.debug_accel(4).tobytes(), c.rotation_info()["per_pass"], c.accel_info()["stack4_entries"])
        q_rot = c.accel_quality()
    r_plain, r_rot = q_plain["cost"] / q_plain["built_cost"], q_rot["cost"] / q_rot["built_cost"]
    print(f"cost / built cost: refitted {r_plain:.4f}, refitted and rotated {r_rot:.4f}")
    assert n > 0 and 1.0 < r_rot < r_plain
    with context(evplp) as c:
        room.upload(c)
        c.set_refit_rotations(2)
        assert c.rotation_info()["refit_passes"] == 2
        apply(c, mo); c.refit_accel()
        got = (c.debug_accel(0).tobytes(), c.debug_accel(4).tobytes(), c.rotation_info()["per_pass"], c.accel_info()["stack4_entries"])
        assert got == want
        q = c.accel_quality()
        assert q["last_action"] == 3 and q["cost"] == q_rot["cost"] and c.refit_info()["refits"] == 1 and c.rotation_info()["since_build"] == n
        same(render(evplp, c), render_fresh(evplp, scattered), "the rotating refit")
        c.set_refit_rotations(0)                                              # off again: the plain refit, and it keeps the rotated topology
        apply(c, mo); c.refit_accel()
        assert c.debug_accel(0).tobytes() == want[0] and c.rotation_info()["last_call"] == n
    # with a policy the ratio is applied to the cost AFTER the rotations: a ratio between the two keeps the rotated tree and rebuilds the plain one
    between = 0.5 * (r_plain + r_rot)
    for rot, ratio, action in ((2, between, 3), (0, between, 2), (2, 0.5 * (1.0 + r_rot), 2), (0, 2.0 * r_plain, 1), (2, 2.0 * r_plain, 3)):
        with context(evplp) as c:
            room.upload(c)
            c.set_refit_policy(ratio)
            c.set_refit_rotations(rot)
            apply(c, mo); c.refit_accel()
            q, ri = c.accel_quality(), c.rotation_info()
            assert q["last_action"] == action, (rot, ratio, q)
            assert q["policy_rebuilds"] == (1 if action == 2 else 0)
            assert ri["last_call"] == (n if rot else 0) and ri["since_build"] == (n if action == 3 else 0)
            if action == 3:
                assert q["cost"] == q_rot["cost"] and c.debug_accel(0).tobytes() == want[0]


def render_fresh(evplp, scattered):
    with context(evplp) as c:
        scattered.upload(c)
        return render(evplp, c)


# ---- 6
def test_deep_trees(evplp):
    DW, DH, N = 64, 48, 200
    sd = scenes.morton_chain(aspect=DW / DH)

    def ctx(builder):
        c = evplp.Context(DW, DH, N, N, P, bvh_builder=builder, deterministic=True)
        sd.upload(c)
        return c

    def frame(c):
        c.primary(JITTER, clear_light=True); c.trace_light_paths(7)
        return [c.download(b)[:DH].tobytes() for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG, evplp.BUF_LIGHT)] + [c.download(evplp.BUF_RECORDS).tobytes()]

    with ctx(1) as c:
        want = frame(c)
    with ctx(0) as c:                                                         # the host LBVH: a chain of two dozen levels
        info0, nodes0 = c.accel_info(), c.debug_accel(0)
        levels0 = wr.tree_levels(nodes0)
        assert info0["builder"] == "lbvh" and levels0 >= 20
        twin = evplp.rotate_tree(nodes0, c.debug_accel(3), soup_of(sd), 3)
        n = c.optimize_accel(3)
        # before any launch over the rotated tree: the bounds the walks rely on, on the downloaded nodes
        info, nodes, n4 = c.accel_info(), c.debug_accel(0), c.debug_accel(4)
        print(f"morton chain, host LBVH: {len(nodes)} nodes, depth {info0['depth']}, levels {levels0} -> {wr.tree_levels(nodes)}, rotations {twin['rotations']}, stack4_entries {info0['stack4_entries']} -> {info['stack4_entries']}")
        assert n == sum(twin["rotations"]) > 0 and np.array_equal(refs(nodes), twin["children"])
        assert info["depth"] <= info0["depth"] and wr.tree_levels(nodes) <= levels0 <= info["depth"]
        assert np.array_equal(n4["child"], wr.four_wide(nodes)["child"])
        worst, generic = wr.worst_case_entries(n4), 3 * ((info["depth"] + 1) // 2) + 4
        assert info["stack4_entries"] == worst + 2 and worst <= min(info["stack4_entries"], generic)
        eye, dirs = wr.primary_rays(sd, DW, DH, JITTER)
        sp = wr.replay_closest(n4, np.broadcast_to(eye, (DW * DH, 3)), dirs.reshape(-1, 3), 0.1, 100.0)
        packet = max(wr.replay_packet(nodes, eye, dirs[y:y + 8, x:x + 8].reshape(-1, 3), 0.1, 100.0) for y in range(0, DH, 8) for x in range(0, DW, 8))
        assert sp.max() <= worst and packet <= wr.tree_levels(nodes) - 1 <= 62
        got = frame(c)
    assert got == want, "G-buffer or light-path records over the rotated chain differ from the SAH tree's"


# ---- 7
def test_refusals_leave_the_context_usable(evplp, room, scattered):
    with context(evplp) as c:
        with pytest.raises(evplp.EvplpError) as e:                            # no accel built
            c.optimize_accel(1)
        assert e.value.status == evplp.ERR_INVALID
        for bad in (-1, 9):
            with pytest.raises(evplp.EvplpError) as e:
                c.set_refit_rotations(bad)
            assert e.value.status == evplp.ERR_INVALID
        room.upload(c)
        for bad in (0, 9, -3):
            with pytest.raises(evplp.EvplpError) as e:
                c.optimize_accel(bad)
            assert e.value.status == evplp.ERR_INVALID and "1 .. 8" in str(e.value)
        apply(c, motion_scatter(room))                                        # dirty: refused like a pass
        with pytest.raises(evplp.EvplpError) as e:
            c.optimize_accel(1)
        assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value) and "evplp_build_accel" in str(e.value)
        assert c.rotation_info() == {"since_build": 0, "last_call": 0, "per_pass": [0] * 8, "refit_passes": 0}
        c.refit_accel()
        assert evplp.lib().evplp_optimize_accel(c._h, 1, None) == evplp.OK        # (the count is optional)
        assert c.rotation_info()["last_call"] > 0
        same(render(evplp, c), render_fresh(evplp, scattered), "after the refusals")
        c.build_accel()                                                       # a build starts the count again
        assert c.rotation_info()["since_build"] == 0 and c.accel_quality()["last_action"] == 0


@pytest.mark.parametrize("partition", ["strips", "iterations"])
def test_group(evplp, room, scattered, partition):
    mo = motion_scatter(room)
    js = [JITTER, (-0.003, 0.002)]

    def fparams(total, seed):
        return evplp.frame_params(camera_pos=room.cam_origin, mis_mode=1, pdf_mc=0.4, clamping_value=1.0 / total, photon_radius=0.3, num_light_paths=NPATHS,
                                  num_vpl_light_paths=NPATHS, photons_per_path=P, do_accumulate=1, rng_seed=seed, jitter=JITTER)

    with aged(evplp, room, "sah") as c:
        n = c.optimize_accel(2)
        per_pass = c.rotation_info()["per_pass"]
        _, total, _ = c.scene_metrics()
        c.clear_accumulators()
        for i in range(2):
            fp = fparams(total, 7 + i)
            c.primary(js[i]); c.trace_light_paths(7 + i); c.gather_vpl(fp); c.splat_photons(fp)
        want = c.resolve(0.5, 0.5, 1.0)[:H]
    assert n > 0 and want.max() > 0
    kw = {} if partition == "strips" else {"partition": "iterations"}
    with evplp.Group(W, H, NPATHS, NPATHS, P, 2, devices=[0, 0], deterministic=True, **kw) as g:
        for r in range(2):
            room.upload(g.rank(r))
        for bad in (0, 9):
            with pytest.raises(evplp.EvplpError) as e:                        # refused on the caller's thread: the group stays usable
                g.optimize_accel(bad)
            assert e.value.status == evplp.ERR_INVALID
        with pytest.raises(evplp.EvplpError):
            g.set_refit_rotations(9)
        if partition == "strips":                                             # the call of its own ...
            for m, v in mo.items():
                g.update_mesh(m, v)
            with pytest.raises(evplp.EvplpError) as e:                        # (dirty)
                g.optimize_accel(2)
            assert e.value.status == evplp.ERR_INVALID
            g.refit_accel()
            assert g.optimize_accel(2) == n
        else:                                                                 # ... and inside the group's refit
            g.set_refit_rotations(2)
            for m, v in mo.items():
                g.update_mesh(m, v)
            g.refit_accel()
        assert all(g.rank(r).rotation_info()["per_pass"] == per_pass and g.rank(r).rotation_info()["last_call"] == n for r in range(2))
        g.clear_accumulators()
        for i in range(2):
            if partition == "iterations":
                g.select_rank(i)
            fp = fparams(total, 7 + i)
            g.primary(js[i]); g.trace_light_paths(7 + i); g.gather(fp, 0); g.splat_photons(fp)
        got = g.resolve(0.5, 0.5, 1.0)
    if partition == "strips":
        assert got.tobytes() == want.tobytes()
    else:
        assert np.linalg.norm(got.astype(np.float64) - want) / np.linalg.norm(want.astype(np.float64)) < 1e-6
