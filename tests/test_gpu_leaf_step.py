"""The hand-written leaf step of the packet walks (device_common.hpp: EV_PAIR_TEXT, EV_WALK_LOOP_ASM).

1. evplp_selftest(2): the assembly triangle-pair test against tri_pair_test, its C++ statement, on the same device-generated inputs
   (classes: random; small integers with rays through vertices, along edges and ending exactly on tmin / tmax; rays in the plane;
   denormal denominators; an all-zero B half; coordinates at 1e-15 .. 1e15), for both register layouts the walks use.
2. Hand-made meshes of 1, 2, 3, 4, 5 and 9 triangles -- leaves of every count 1 .. 4 -- under eight uploaded VPLs over an uploaded
   24 x 16 G-buffer: per VPL the lit / unlit pixel sets, the shadow-ray count and the unoccluded-pair count of gather_vpl equal the
   oracle's, with the entry cuts and from the root, and gather_vsl's walk agrees on the same scenes.
"""
import math

import numpy as np
import pytest

import oracle_api as oa
import scenes

pytestmark = pytest.mark.gpu

W, H = 24, 16
NPATHS, P = 2, 4            # 8 record slots

# Two layers of one 12 x 8 rectangle cut along its two diagonals: four triangles with the same bounding rectangle that cover different
# halves of it (the SAH builder keeps triangles whose boxes coincide in ONE leaf -- a split saves no area), so that a segment is
# stopped by one triangle of one pair only, whichever pair the builder puts first.  Then a triangle off to the side, then four
# more at other heights and tilts.
TRIS = [
    [(2, 2, 1.0), (14, 2, 1.0), (2, 10, 1.0)],
    [(2, 2, 1.1), (14, 2, 1.1), (14, 10, 1.1)],
    [(14, 10, 1.0), (2, 10, 1.0), (14, 2, 1.0)],
    [(2, 2, 1.1), (14, 10, 1.1), (2, 10, 1.1)],
    [(17, 3, 2.0), (22, 3, 2.0), (17, 8, 2.0)],
    [(16, 10, 0.5), (23, 11, 0.75), (18, 15, 1.5)],
    [(1, 12, 2.5), (6, 12, 2.0), (3, 15, 3.0)],
    [(8, 11, 0.25), (12, 12, 0.25), (9, 15, 0.5)],
    [(19, 0, 1.0), (23, 1, 3.0), (20, 2, 1.5)],
]
# above the rectangle; off to the side; BETWEEN its two layers (only the lower one is in the way); grazing from the left (long shadows:
# whole tiles occluded); below every occluder (nothing in the way: empty entry cuts); grazing from the far corner; high above a
# corner; low above both layers (a shadow wider than the rectangle)
VPLS = [(8, 6, 4), (20, 12, 4), (8.25, 6.25, 1.05), (-10, 6, 2), (8, 6, 0.125), (30, 20, 1.5), (3, 3, 8), (12, 8, 1.25)]


def make_scene(ntri):
    s = scenes.SceneData()
    s.aspect = W / H
    m = s.add_material((0, 0, 0))
    verts = np.asarray(TRIS[:ntri], np.float32).reshape(-1, 3)
    s.light_mesh = s.add_mesh(verts, np.arange(3 * ntri).reshape(-1, 3), m)      # (a scene needs a light mesh: the occluders are it)
    s.cam_origin = [12.0, 8.0, 20.0]; s.cam_lookat = [12.0, 8.0, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.triangle_soup()
    return s


def make_inputs():
    """the receiver: the plane z = 0 seen through a 24 x 16 G-buffer (one world unit per pixel), white, facing up"""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32) + 0.5, np.arange(W, dtype=np.float32) + 0.5, indexing="ij")
    pos = np.stack([xs, ys, np.zeros_like(xs), np.ones_like(xs)], -1).astype(np.float32)
    nrm = np.zeros((H, W, 4), np.float32); nrm[..., 2] = 1.0
    dif = np.ones((H, W, 4), np.float32)
    phg = np.zeros((H, W, 4), np.float32)
    gbuf = [pos, nrm, dif, phg, np.zeros((H, W, 4), np.float32)]
    rec = np.zeros(NPATHS * P, dtype=oa.RECORD_DTYPE)
    rec["pos"] = np.asarray(VPLS, np.float32)
    rec["normal"] = (0, 0, -1); rec["flux_dir"] = (0, 0, -1)
    rec["flux"] = 1.0; rec["rho_d"] = 1.0; rec["p_select_lambert"] = 1.0
    return gbuf, rec


def upload_inputs(ctx, evplp, gbuf, records):
    for b, plane in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG), gbuf):
        pad = np.zeros((ctx.local_rows, W, 4), np.float32); pad[:H] = plane
        ctx.upload(b, pad)
    ctx.upload(evplp.BUF_RECORDS, records)


@pytest.fixture(scope="module")
def reference(oracle):
    """per mesh: the scene, and per VPL the oracle's image, shadow-ray count and unoccluded-pair count (computed once)"""
    gbuf, rec = make_inputs()
    out = {}
    for ntri in (1, 2, 3, 4, 5, 9):
        sd = make_scene(ntri)
        osc = oa.Scene(sd)
        per_vpl = []
        for k in range(len(VPLS)):
            r = rec.copy(); r["flags"][k] = 1
            kw = dict(camera_pos=sd.cam_origin, mis_mode=0, num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
            img, _ = osc.gather(oa.frame_params(**kw), W, H, gbuf, r)
            per_vpl.append((r, img[..., :3].sum(-1) > 0, osc.gather_counts(oa.frame_params(**kw), W, gbuf, r, np.arange(H))))
        out[ntri] = (sd, osc, per_vpl)
    return gbuf, out


def test_pair_asm_matches_tri_pair_test(evplp):
    with evplp.Context(W, H, NPATHS, NPATHS, P) as c:
        r = [int(x) for x in c.selftest(2)]
    mismatches, cases, hits = r[0], r[1], r[2]
    per_class = [r[3] & 0xffffffff, r[3] >> 32, r[4] & 0xffffffff, r[4] >> 32, r[5] & 0xffffffff, r[5] >> 32]
    print("selftest(2): mismatches", mismatches, "cases", cases, "hits", hits, "per class", per_class)
    assert cases == 2 * 4096 * 64 * 2          # both register layouts, two triangles per lane
    assert mismatches == 0
    assert hits == sum(per_class) and hits > 0
    # every class aims its lanes at points of its triangles, a third of them interior or on an edge at a t inside the range: a class
    # without hits (or with all of them) would compare nothing
    per_class_cases = cases // 6
    for k, n in enumerate(per_class):
        assert per_class_cases // 100 <= n <= per_class_cases // 2, (k, n, per_class_cases)


@pytest.mark.parametrize("cuts", [True, False], ids=["cuts", "root"])
@pytest.mark.parametrize("ntri", [1, 2, 3, 4, 5, 9])
def test_small_scene_visibility(evplp, reference, monkeypatch, ntri, cuts):
    gbuf, ref = reference
    sd, osc, per_vpl = ref[ntri]
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    if not cuts:
        monkeypatch.setenv("EVPLP_CUTS", "0")       # (read when the context is created: every walk starts at the root)
    kw = dict(camera_pos=sd.cam_origin, mis_mode=0, num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
    seen = {"lit_tile": 0, "dark_tile": 0, "split_tile": 0}
    with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=evplp.BVH_SAH, deterministic=True) as c:
        sd.upload(c)
        info = c.accel_info()
        if ntri <= 4:
            assert info["leaves"] == 1, info        # one leaf of ntri triangles under a root with an absent child
        for k, (rec, lit_ref, counts) in enumerate(per_vpl):
            upload_inputs(c, evplp, gbuf, rec)
            c.clear_accumulators()
            c.gather_vpl(evplp.frame_params(**kw))
            got = c.download(evplp.BUF_VPL_ACCUM)[:H]
            st = c.pass_stats(evplp.PASS_GATHER_VPL)
            lit = got[..., :3].sum(-1) > 0
            assert np.array_equal(lit, lit_ref), (ntri, k, np.argwhere(lit != lit_ref)[:8].tolist())
            assert (st["rays"], st["shaded"]) == counts, (ntri, k, st["rays"], st["shaded"], counts)
            assert st["rays"] == W * H
            for ty in range(0, H, 8):
                for tx in range(0, W, 8):
                    t = lit_ref[ty:ty + 8, tx:tx + 8]
                    seen["lit_tile" if t.all() else "dark_tile" if not t.any() else "split_tile"] += 1
    # the placements give every kind of 8 x 8 tile: no lane occluded, every lane occluded, and both within one packet
    assert seen["lit_tile"] > 0 and seen["split_tile"] > 0 and (ntri < 3 or seen["dark_tile"] > 0), seen


@pytest.mark.parametrize("ntri", [1, 2, 3, 4, 5, 9])
def test_small_scene_vsl_walk(evplp, reference, ntri):
    gbuf, ref = reference
    sd, osc, per_vpl = ref[ntri]
    r = 0.25
    kw = dict(camera_pos=sd.cam_origin, vsl_radius=r, vsl_inv_pi_radius2=1.0 / (math.pi * r * r), num_light_paths=NPATHS, num_vpl_light_paths=NPATHS,
              photons_per_path=P, rng_seed=9)
    rec = per_vpl[0][0].copy(); rec["flags"] = 1
    with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=evplp.BVH_SAH, deterministic=True) as c:
        sd.upload(c)
        upload_inputs(c, evplp, gbuf, rec)
        c.clear_accumulators()
        c.gather_vsl(evplp.frame_params(**kw))
        got = c.download(evplp.BUF_VPL_ACCUM)[:H]
        pairs = c.pass_stats(evplp.PASS_GATHER_VSL)["pairs"]
    want, ref_pairs = osc.gather(oa.frame_params(**kw), W, H, gbuf, rec, vsl=True)
    assert pairs == ref_pairs and want[..., :3].max() > 0
    assert np.array_equal(got[..., :3].sum(-1) > 0, want[..., :3].sum(-1) > 0)
    # (the bar of test_gather_vsl: the estimators branch on sampled directions, a 1-ulp difference may flip one sample term of a pair)
    g, w = got[..., :3].astype(np.float64), want[..., :3].astype(np.float64)
    assert np.sqrt(((g - w) ** 2).sum()) <= 1e-3 * np.sqrt((w ** 2).sum())
