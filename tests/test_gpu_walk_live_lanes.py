"""The packet walk with EXEC = its live lanes (device_common.hpp: occluded_wave, EV_SYN_VISIT_ASM_, EV_WALK_LOOP_ASM).

1. evplp_selftest(5): the whole hand-written walk against occluded_wave_ref, the C++ walk, on device-generated packets through a
   device-generated tree, for eight patterns of lanes that start alive (all; all but lane 0; either half; only lane 63; only lane 0; a
   random quarter; none).
2. Small gathers in the pattern of test_gpu_leaf_step.py -- an uploaded G-buffer (the plane z = 0, one world unit per pixel, lane =
   8 * (y % 8) + x % 8 of its 8 x 8 tile), eight uploaded VPLs, hand-made meshes -- chosen for what the lanes of a packet do:
   stencil_row / backface_row  the first eight lanes of every tile are dead from the start (w = 0; normals that face away): the
                 in-place visit's v_readfirstlane reads from lane 8
   half          under VPL 0, straight above tile (0, 0): rectangle A shadows exactly lanes 0-31 of that tile, B1 eight and B2 four of
                 lanes 32-63.  The child more lanes enter is descended first, so A's leaf is the first one tested and takes half the
                 packet out of EXEC; the other half goes on to B1 and B2, which it enters both (a push, a hit, a pop, a hit)
   all           one rectangle over everything: every lane dies at the first leaf
   none          a triangle whose box holds the image and whose area no segment reaches: every lane tests it, none dies
   ragged        `half` in a 21 x 13 frame: tiles with off-image lanes
   Per scene and VPL the lit / unlit pixel sets, the shadow-ray count and the unoccluded-pair count equal the oracle's, with entry cuts
   and with EVPLP_CUTS=0, for gather_vpl and for gather_vsl's walk, and the accumulators are byte-equal between cuts and no cuts.
   The lane patterns themselves are confirmed with the oracle alone (lane_patterns, asserted in the reference fixture).
"""
import math

import numpy as np
import pytest

import oracle_api as oa
import scenes

pytestmark = pytest.mark.gpu

NPATHS, P = 2, 4            # 8 record slots
R_VSL = 0.25


def rect(x0, x1, y0, y1, z):
    """two triangles with the same bounding rectangle (the SAH builder keeps them in one leaf)"""
    return [[(x0, y0, z), (x1, y0, z), (x0, y1, z)], [(x1, y1, z), (x0, y1, z), (x1, y0, z)]]


# Seen from VPL 0 = (4, 4, 8) a point (x, y, z) lies on the segment to the pixel centre 4 + (x - 4) * 8 / (8 - z) (likewise y):
# A at z = 1 ends at y = 4, between the images 3.5625 and 4.4375 of the pixel rows 3 and 4; B1 at z = 2 starts at y = 5.5, between the images
# 5.125 and 5.875 of rows 5 and 6, and ends at x = 4, between columns 3 and 4; B2 at z = 3 holds the image 4.3125 of row 4 but not 4.9375
# of row 5, and starts at x = 4, between the images 3.6875 and 4.3125 of columns 3 and 4.
A = rect(-2.0, 10.0, -2.0, 4.0, 1.0)
B1 = rect(-2.0, 4.0, 5.5, 8.5, 2.0)
B2 = rect(4.0, 10.0, 4.1, 4.6, 3.0)
MESHES = {
    "half": A + B1 + B2,
    "all": rect(-50.0, 80.0, -50.0, 70.0, 1.0),
    # x + y >= 80 at z = 1: a segment crosses z = 1 at a convex combination of its pixel (x + y <= 40) and its VPL (x + y <= 50)
    "none": [[(100.0, 100.0, 1.0), (100.0, -20.0, 1.0), (-20.0, 100.0, 1.0)]],
}
# name: (W, H, mesh, rows whose lanes are dead from the start, how)
SCENES = {
    "stencil_row": (24, 16, "half", "stencil"),
    "backface_row": (24, 16, "half", "backface"),
    "half": (24, 16, "half", None),
    "all": (24, 16, "all", None),
    "none": (24, 16, "none", None),
    "ragged": (21, 13, "half", None),
}
# straight above tile (0, 0); off to the side; above the middle; grazing from the left (long shadows); below every occluder; grazing from
# the far corner; high above a corner; low above the middle, between the layers
VPLS = [(4, 4, 8), (20, 12, 4), (12, 8, 6), (-10, 6, 2.5), (4, 4, 0.5), (30, 20, 1.5), (3, 3, 8), (12, 8, 2.5)]


def make_scene(tris, W, H):
    s = scenes.SceneData()
    s.aspect = W / H
    m = s.add_material((0, 0, 0))
    verts = np.asarray(tris, np.float32).reshape(-1, 3)
    s.light_mesh = s.add_mesh(verts, np.arange(len(verts)).reshape(-1, 3), m)      # (a scene needs a light mesh: the occluders are it)
    s.cam_origin = [12.0, 8.0, 20.0]; s.cam_lookat = [12.0, 8.0, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.triangle_soup()
    return s


def make_inputs(W, H, dead):
    """the receiver: the plane z = 0 (one world unit per pixel), white, facing up; `dead`: the first row of every tile fails the stencil
    test (w = 0) or faces away from every VPL"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32) + 0.5, np.arange(W, dtype=np.float32) + 0.5, indexing="ij")
    pos = np.stack([xs, ys, np.zeros_like(xs), np.ones_like(xs)], -1).astype(np.float32)
    nrm = np.zeros((H, W, 4), np.float32); nrm[..., 2] = 1.0
    if dead == "stencil":
        pos[0::8, :, 3] = 0.0
    if dead == "backface":
        nrm[0::8, :, 2] = -1.0
    dif = np.ones((H, W, 4), np.float32)
    phg = np.zeros((H, W, 4), np.float32)
    gbuf = [pos, nrm, dif, phg, np.zeros((H, W, 4), np.float32)]
    rec = np.zeros(NPATHS * P, dtype=oa.RECORD_DTYPE)
    rec["pos"] = np.asarray(VPLS, np.float32)
    rec["normal"] = (0, 0, -1); rec["flux_dir"] = (0, 0, -1)
    rec["flux"] = 1.0; rec["rho_d"] = 1.0; rec["p_select_lambert"] = 1.0
    return gbuf, rec


def upload_inputs(ctx, evplp, gbuf, records, W, H):
    for b, plane in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG), gbuf):
        pad = np.zeros((ctx.local_rows, W, 4), np.float32); pad[:H] = plane
        ctx.upload(b, pad)
    ctx.upload(evplp.BUF_RECORDS, records)


def vpl_kw(sd):
    return dict(camera_pos=sd.cam_origin, mis_mode=0, num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)


def vsl_kw(sd):
    return dict(camera_pos=sd.cam_origin, vsl_radius=R_VSL, vsl_inv_pi_radius2=1.0 / (math.pi * R_VSL * R_VSL), num_light_paths=NPATHS,
                num_vpl_light_paths=NPATHS, photons_per_path=P, rng_seed=9)


def lit_of(osc, sd, W, H, gbuf, rec, k):
    """the oracle's lit pixels under VPL k alone"""
    r = rec.copy(); r["flags"][k] = 1
    img, _ = osc.gather(oa.frame_params(**vpl_kw(sd)), W, H, gbuf, r)
    return img[..., :3].sum(-1) > 0


def lane_patterns():
    """With the oracle alone: what the lanes of tile (0, 0) do under VPL 0 in `half` and in `all` (every pixel of the tile is a live lane
    there: on the plane, facing the VPL)."""
    W, H = 24, 16
    gbuf, rec = make_inputs(W, H, None)
    dark = {}
    for name, tris in (("A", A), ("B1", B1), ("B2", B2), ("half", MESHES["half"]), ("all", MESHES["all"])):
        sd = make_scene(tris, W, H)
        dark[name] = ~lit_of(oa.Scene(sd), sd, W, H, gbuf, rec, 0)[:8, :8]
    lanes = {n: set(np.flatnonzero(d.reshape(-1)).tolist()) for n, d in dark.items()}
    assert lanes["A"] == set(range(32)), sorted(lanes["A"])                       # one half of the packet, at one leaf
    assert len(lanes["B1"]) == 8 and len(lanes["B2"]) == 4 and lanes["B1"] | lanes["B2"] <= set(range(32, 64)) and not (lanes["B1"] & lanes["B2"])
    assert lanes["half"] == lanes["A"] | lanes["B1"] | lanes["B2"]                # ... and twenty lanes stay alive to the end
    assert lanes["all"] == set(range(64))
    return lanes


@pytest.fixture(scope="module")
def reference(oracle):
    """per scene: the inputs, the scene, and per VPL the oracle's lit image, shadow-ray and unoccluded-pair counts, and the VSL gather's lit
    image and pair count (computed once)"""
    lane_patterns()
    out = {}
    for name, (W, H, mesh, dead) in SCENES.items():
        gbuf, rec0 = make_inputs(W, H, dead)
        sd = make_scene(MESHES[mesh], W, H)
        osc = oa.Scene(sd)
        per_vpl = []
        for k in range(len(VPLS)):
            r = rec0.copy(); r["flags"][k] = 1
            img, _ = osc.gather(oa.frame_params(**vpl_kw(sd)), W, H, gbuf, r)
            counts = osc.gather_counts(oa.frame_params(**vpl_kw(sd)), W, gbuf, r, np.arange(H))
            vimg, vpairs = osc.gather(oa.frame_params(**vsl_kw(sd)), W, H, gbuf, r, vsl=True)
            per_vpl.append((r, img[..., :3].sum(-1) > 0, counts, vimg[..., :3].sum(-1) > 0, vpairs))
        out[name] = (W, H, gbuf, sd, per_vpl)
    # what the scenes are for, in the oracle's own numbers (rays, unoccluded pairs) under VPL 0
    n_dead = 24 * 2
    assert out["half"][4][0][2][0] == 24 * 16 and out["stencil_row"][4][0][2][0] == 24 * 16 - n_dead and out["backface_row"][4][0][2][0] == 24 * 16 - n_dead
    assert out["all"][4][0][2] == (24 * 16, 0)
    assert all(c[2][0] > 0 and c[2][1] == c[2][0] for c in out["none"][4])
    assert out["ragged"][4][0][2][0] == 21 * 13
    return out


def test_walk_asm_matches_the_cpp_walk(evplp):
    with evplp.Context(24, 16, NPATHS, NPATHS, P) as c:
        r = [int(x) for x in c.selftest(5)]
    mismatches, cases, occluded = r[0], r[1], r[2]
    per_class = [(r[3 + k // 3] >> (21 * (k % 3))) & 0x1fffff for k in range(8)]
    print("selftest(5): mismatches", mismatches, "cases", cases, "occluded", occluded, "per class", per_class)
    assert cases == 4096 * 64
    assert mismatches == 0
    assert occluded == sum(per_class)
    alive = [64, 63, 32, 32, 1, 1, 16, 0]              # lanes that start alive per packet (class 6: on average)
    for k, n in enumerate(per_class):
        # every class but "none" is exercised: some of its live lanes are occluded, and not all of them
        assert (n == 0) if k == 7 else (0 < n < 512 * alive[k]), (k, n)


@pytest.mark.parametrize("name", list(SCENES))
def test_live_lane_scenes(evplp, reference, monkeypatch, name):
    W, H, gbuf, sd, per_vpl = reference[name]
    acc = {}
    for cuts in (True, False):
        monkeypatch.delenv("EVPLP_CUTS", raising=False)
        if not cuts:
            monkeypatch.setenv("EVPLP_CUTS", "0")       # (read when the context is created: every walk starts at the root)
        with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=evplp.BVH_SAH, deterministic=True) as c:
            sd.upload(c)
            for k, (rec, lit_ref, counts, vlit_ref, vpairs) in enumerate(per_vpl):
                upload_inputs(c, evplp, gbuf, rec, W, H)
                c.clear_accumulators()
                c.gather_vpl(evplp.frame_params(**vpl_kw(sd)))
                got = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
                st = c.pass_stats(evplp.PASS_GATHER_VPL)
                lit = got[..., :3].sum(-1) > 0
                assert np.array_equal(lit, lit_ref), (name, cuts, k, np.argwhere(lit != lit_ref)[:8].tolist())
                assert (st["rays"], st["shaded"]) == counts, (name, cuts, k, st["rays"], st["shaded"], counts)
                c.clear_accumulators()
                c.gather_vsl(evplp.frame_params(**vsl_kw(sd)))
                vgot = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
                pairs = c.pass_stats(evplp.PASS_GATHER_VSL)["pairs"]
                vlit = vgot[..., :3].sum(-1) > 0
                assert np.array_equal(vlit, vlit_ref), (name, cuts, k, np.argwhere(vlit != vlit_ref)[:8].tolist())
                assert pairs == vpairs, (name, cuts, k, pairs, vpairs)
                acc[(cuts, k)] = (got, vgot)
    for k in range(len(per_vpl)):
        assert acc[(True, k)][0].tobytes() == acc[(False, k)][0].tobytes(), (name, k, "gather_vpl: cuts change a bit")
        assert acc[(True, k)][1].tobytes() == acc[(False, k)][1].tobytes(), (name, k, "gather_vsl: cuts change a bit")
