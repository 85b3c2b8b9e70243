"""Ray queries on the device against the brute force, on the inputs the walk's error budget does not obviously cover: origins 1e2 to 1e4
scene sizes away, directions scaled by 2^+-60 (and 2^+-100, which the kernels refuse), oblique soups -- one far from the origin, one a
thousandth and one a thousand times the size -- a scene without thickness and the box room's axis-aligned outlines.

ray_hostile.py builds the batches, the references (evo_closest_brute / evo_occluded_brute for every ray) and the condition under which a
ray is compared byte for byte; test_ray_query_hostile_host.py holds the share that condition sets aside under 0.5 % per (scene, kind)
without a GPU.  Here every decidable ray must equal the brute force in triangle, t, beta and gamma (or the occlusion byte), every ray set
aside must carry a triangle the triangle test accepts with the reported t bits, or a miss, and every invalid ray is refused.

Against the kernels as they were before the far-origin slack (device_common.hpp slab_near<FAR>) and the direction range (ray_valid), the
closest-hit test on the SAH tree failed on all six scenes: far 100 / 1000 / 10000 gave 8 / 13 / 6 wrong rays on the flat scene (a
higher-numbered triangle of equal t: the lower one's box was culled) and 2 / 6 / 3 in the room, far 10000 gave 25 on the soup far from
the origin (25 to 34 over the five builders, 2 to 10 per far kind on the flat scene under the device LBVH and PLOC), and every scene's 400
rays scaled by 2^+-100 were walked instead of refused.  The soups at the origin, the 2^+-60 kinds, the ordering pass, the rotated mesh and
evplp_primary on the miniature passed there as they do now."""
import copy
import math

import numpy as np
import pytest

import oracle_api as oa
import ray_hostile as rh
import walk_replay as wr
from test_gpu_ray_query import BUILDERS, NP, P, H, W

pytestmark = pytest.mark.gpu

F = np.float32


def say(*a):
    print("[hostile rays]", *a, flush=True)


@pytest.fixture(scope="module")
def batches(oracle):
    return {name: rh.Hostile(rh.make_scene(name)) for name in rh.SCENES}


def context(evplp, sd, builder=1):
    c = evplp.Context(W, H, NP, NP, P, bvh_builder=builder, deterministic=True)
    sd.upload(c)
    return c


def check_all(c, b, what):
    """closest hit with each filter and occlusion of the whole batch against the references"""
    for filt in (0, 1, 2):
        hits = c.trace_closest(b.rays, filt)
        b.check_closest(hits, filt, f"{what}, filter {filt}")
        inv = hits[b.invalid]
        assert (inv["triangle"] == -2).all() and (inv["t"] == 0).all() and (inv["beta"] == 0).all() and (inv["gamma"] == 0).all(), (what, filt)
        assert (hits["triangle"][b.valid] >= -1).all(), (what, filt)
    out = c.trace_occluded(b.rays)
    b.check_occluded(out, f"{what}, occlusion")
    assert (out[b.invalid] == 2).all() and (out[b.valid] < 2).all(), what


# ---- 1: the SAH tree on every scene
@pytest.mark.parametrize("scene", rh.SCENES)
def test_closest_hit_with_each_filter_and_occlusion_match_the_brute_force(evplp, batches, scene):
    b = batches[scene]
    with context(evplp, b.sd) as c:
        assert c.accel_info()["builder"] == "sah"
        check_all(c, b, scene)
    say(f"{scene}: S = {b.S:.4g}, {int((b.brute[0]['triangle'] >= 0).sum())} hit, {len(b.invalid)} refused, set aside {[int(b.aside[f].sum()) for f in (0, 1, 2)]}")


# ---- 2: every builder against the reference, not against another builder
@pytest.mark.parametrize("scene,builder", [(s, k) for s in ("soup", "soup far away") for k in sorted(BUILDERS)] + [("flat", 3), ("flat", 4)])
def test_every_builders_tree_gives_the_brute_forces_answers(evplp, batches, scene, builder):
    b = batches[scene]
    with context(evplp, b.sd, builder) as c:
        assert c.accel_info()["builder"] == BUILDERS[builder]
        check_all(c, b, f"{scene}, {BUILDERS[builder]}")


# ---- 3: the ordering pass (its keys clamp a far origin to the box's border: that may change the launch order and nothing else)
@pytest.mark.parametrize("scene", rh.SCENES)
def test_the_ordering_pass_changes_no_byte_on_far_origins(evplp, batches, scene):
    b = batches[scene]
    with context(evplp, b.sd) as c:
        for filt in (0, 1, 2):
            assert c.trace_closest(b.rays, filt, order=True).tobytes() == c.trace_closest(b.rays, filt).tobytes(), (scene, filt)
        assert c.trace_occluded(b.rays, order=True).tobytes() == c.trace_occluded(b.rays).tobytes(), scene


# ---- 4: a moved scene: the refit recomputes the pad (scene_fold), here over oblique boxes
def test_a_rotated_mesh_is_hit_where_the_refit_left_it(evplp, oracle, batches):
    sd = batches["soup"].sd
    mesh = 1
    a = math.radians(33.0)
    k = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + math.sin(a) * K + (1.0 - math.cos(a)) * (K @ K)
    m = np.concatenate([R, np.array([[2.5], [-1.0], [1.5]])], axis=1).astype(F)
    with context(evplp, sd) as c:
        c.transform_mesh(mesh, m.reshape(12))
        c.refit_accel()
        moved = copy.deepcopy(sd)
        for i in range(len(moved.meshes)):
            moved.meshes[i]["verts"] = c.mesh_vertices(i, 0)
        assert not np.array_equal(moved.meshes[mesh]["verts"], sd.meshes[mesh]["verts"])
        want = (sd.meshes[mesh]["verts"].astype(np.float64) @ R.T + m[:, 3].astype(np.float64))
        assert np.abs(moved.meshes[mesh]["verts"] - want).max() < 1e-4
        moved.triangle_soup()
        b = rh.Hostile(moved, seed=17, n_rays=1024 + rh.N_FAR, far=(1e3,), scaled=False, classic_invalid=False)
        for kind in ("near", "far 1000"):
            assert b.share_aside(kind) <= rh.CAP, (kind, b.share_aside(kind))
        first = sum(len(mm["idx"]) for mm in moved.meshes[:mesh]); count = len(moved.meshes[mesh]["idx"])
        w = b.brute[0]["triangle"]
        assert ((w >= first) & (w < first + count)).sum() > 100, "rays reach the moved mesh"
        check_all(c, b, "soup with a rotated mesh")
        with context(evplp, sd) as c0:
            assert c0.trace_closest(b.rays).tobytes() != c.trace_closest(b.rays).tobytes(), "the query follows the refit"


# ---- 5: the packet walk of evplp_primary on the miniature
@pytest.mark.parametrize("distance", [1.0, 2.0, 3.0])
def test_primary_on_the_miniature_soup_matches_the_brute_force(evplp, oracle, batches, distance):
    """The 1e-3 soup (S = 0.017) seen from 1, 2 and 3 units: |o| / S = 58 to 173.  The frame's rays have tmin 0.1 and tmax 100 in depth."""
    b = batches["soup 1e-3"]
    sd = copy.deepcopy(b.sd)
    centre = 0.5 * (b.lo + b.hi)
    away = np.array([1.0, -0.7, 0.5]); away /= np.linalg.norm(away)
    sd.cam_origin = [float(x) for x in (centre + distance * away).astype(F)]
    sd.cam_lookat = [float(x) for x in centre.astype(F)]
    sd.cam_up = [0.0, 0.0, 1.0]
    sd.fovy = 2.0 * math.atan(0.5 * np.linalg.norm(b.hi - b.lo) / distance)           # the soup's bounding sphere fills the frame's height
    jitter = (0.003, -0.002)
    with evplp.Context(W, H, NP, NP, P, deterministic=True) as c:
        sd.upload(c)
        c.primary(jitter, clear_light=True)
        got = [c.download(x)[:H] for x in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG, evplp.BUF_LIGHT)]
    osc = oa.Scene(sd)
    ref = osc.primary(W, H, jitter, brute=True)
    # the rule of ray_hostile.py per pixel, for the scene's ray (jittered, filter 1) and the light's (not jittered, filter 2)
    aside = np.zeros(W * H, bool)
    for j, filt in ((jitter, 1), ((0.0, 0.0), 2)):
        eye, dirs = wr.primary_rays(sd, W, H, j)
        rays = rh.rays_of(np.broadcast_to(eye, (W * H, 3)), dirs.reshape(-1, 3), 0.1, 100.0)
        win = osc.closest_brute(rays, filt)["triangle"]
        hit = win >= 0
        k = np.where(hit, win, 0)
        aside |= hit & ~rh.crosses_box(rays, b.P[k].min(axis=1), b.P[k].max(axis=1))
        if filt == 1:
            covered = float(hit.mean())
    aside = aside.reshape(H, W)
    assert aside.mean() <= rh.CAP, int(aside.sum())
    assert covered > 0.05, covered
    bad = {n: int(((g.view(np.uint32) != r.view(np.uint32)).any(axis=-1) & ~aside).sum()) for n, g, r in zip(("position", "normal", "diffuse", "phong", "light"), got, ref)}
    say(f"miniature from {distance:g}: {100 * covered:.0f} % of the pixels covered, {int(aside.sum())} set aside, pixels that differ {bad}")
    assert not any(bad.values()), bad
