"""The in-place visit of a synthetic node of an entry cut (device_common.hpp EV_SYN_VISIT_ASM_: the node goes from the slot's LDS copy
straight into the visit's registers; only its two child references become scalars).

1. evplp_selftest(3): the in-place statement against the scalar-operand visit (selftest.hip EV_WALK_VISIT_ASM_) on the same device-generated nodes and
   rays -- both entered-lane masks, the next node, the stack pointer and the whole stack register -- in six classes (random boxes around
   random segments; an absent second entry as the cut kernel writes an odd count; dead lanes among live ones; a box that ends exactly at
   a segment end point; zero half-sizes; coordinates at 1e-15 .. 1e15).
2. A hand-made scene whose cuts hold several entries: 50 small separate triangles in a 10 x 5 grid above a 40 x 24 G-buffer plane (3 x 2
   cut groups, the right column and the lower row ragged; the builder pairs neighbouring triangles: 30 leaves), under eight uploaded
   VPLs -- high above the grid (the pyramid of a whole group holds a dozen triangles and more: the cut is full), oblique from four sides
   (the pyramids graze rows of triangles: other counts), close above the grid, and below every triangle (empty cuts).  Per VPL the
   lit / unlit pixel sets, the shadow-ray count and the unoccluded-pair count equal the oracle's, and the accumulator with cuts is
   byte-equal to the one from the root.

What the counters build showed for this scene (make stats, evplp_debug_counters; one cut group's pixels stencilled in at a time, so that
synthetic visits / walks is the node count of that group's slot; no walk ended early): synthetic nodes per slot, VPL by VPL, the six
groups row by row --
   4 4 2 3 3 2 | 4 4 3 3 3 2 | 2 4 3 1 2 1 | 4 4 2 1 1 0 | 2 2 1 2 3 2 | 4 4 3 0 1 0 | 4 2 2 1 3 2 | 0 0 0 0 0 0
-- slots of one, two, three and four nodes and empty ones all occur.  The counters do not tell an odd entry count from an even one (a
slot of n nodes holds 2 n - 1 or 2 n entries; under VPL 5 one group's walks also visit inner nodes: some of its entries are
subtrees); the absent second entry of an odd count is class 1 of the selftest, and the one-leaf meshes of test_gpu_leaf_step.py
walk a one-entry cut.
"""
import numpy as np
import pytest

import oracle_api as oa
import scenes

pytestmark = pytest.mark.gpu

W, H = 40, 24
NPATHS, P = 2, 4            # 8 record slots


def grid_triangles():
    tris = []
    for j in range(5):
        for i in range(10):
            x, y = 2.0 + 4.0 * i, 2.5 + 5.0 * j - 0.5
            z = 2.0 + 0.125 * ((3 * i + 5 * j) % 7)                     # (heights differ: no two boxes coincide)
            tris.append([(x - 0.75, y - 0.5, z), (x + 0.75, y - 0.5, z + 0.25), (x, y + 0.75, z)])
    return tris


TRIS = grid_triangles()
# high above the middle; high above a corner; oblique from the left, the right, the front and the back; close above the grid; below
# every triangle (nothing in the way: empty cuts)
VPLS = [(20, 12, 30), (2, 2, 25), (-15, 12, 6), (52, 30, 5), (18, -20, 7), (22, 45, 9), (11, 6, 3.5), (20, 12, 0.5)]


def make_scene():
    s = scenes.SceneData()
    s.aspect = W / H
    m = s.add_material((0, 0, 0))
    verts = np.asarray(TRIS, np.float32).reshape(-1, 3)
    s.light_mesh = s.add_mesh(verts, np.arange(3 * len(TRIS)).reshape(-1, 3), m)      # (a scene needs a light mesh: the occluders are it)
    s.cam_origin = [20.0, 12.0, 40.0]; s.cam_lookat = [20.0, 12.0, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.triangle_soup()
    return s


def make_inputs():
    """the receiver: the plane z = 0 seen through a 40 x 24 G-buffer (one world unit per pixel), white, facing up"""
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


def frame_kw(sd):
    return dict(camera_pos=sd.cam_origin, mis_mode=0, num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)


def test_syn_visit_matches_scalar_operand_visit(evplp):
    with evplp.Context(W, H, NPATHS, NPATHS, P) as c:
        r = [int(x) for x in c.selftest(3)]
    mismatches, cases, entered = r[0], r[1], r[2]
    per_class = [r[3] & 0xffffffff, r[3] >> 32, r[4] & 0xffffffff, r[4] >> 32, r[5] & 0xffffffff, r[5] >> 32]
    print("selftest(3): mismatches", mismatches, "cases", cases, "entered", entered, "per class", per_class)
    assert cases == 4096 * 64 * 2              # 64 lanes, two children per node
    assert mismatches == 0
    assert entered == sum(per_class)
    # a class that enters nothing (or everything) compares nothing: between 1 % and 99 % of the lanes of every class, counted for the
    # reference visit
    for k, n in enumerate(per_class):
        class_cases = len(range(k, 4096, 6)) * 128
        assert class_cases // 100 <= n <= class_cases - class_cases // 100, (k, n, class_cases)


def test_grid_scene_with_cuts_equals_root_and_oracle(evplp, oracle, monkeypatch):
    gbuf, rec = make_inputs()
    sd = make_scene()
    osc = oa.Scene(sd)
    kw = frame_kw(sd)
    accum = {}
    for cuts in (True, False):
        monkeypatch.delenv("EVPLP_CUTS", raising=False)
        if not cuts:
            monkeypatch.setenv("EVPLP_CUTS", "0")       # (read when the context is created: every walk starts at the root)
        with evplp.Context(W, H, NPATHS, NPATHS, P, bvh_builder=evplp.BVH_SAH, deterministic=True) as c:
            sd.upload(c)
            assert c.accel_info()["leaves"] > 8                   # (a leaf holds at most four triangles: more leaves than a cut has entries)
            for k in range(len(VPLS)):
                r = rec.copy(); r["flags"][k] = 1
                upload_inputs(c, evplp, gbuf, r)
                c.clear_accumulators()
                c.gather_vpl(evplp.frame_params(**kw))
                accum[cuts, k] = (c.download(evplp.BUF_VPL_ACCUM)[:H].copy(), c.pass_stats(evplp.PASS_GATHER_VPL))
    dark = []
    for k in range(len(VPLS)):
        r = rec.copy(); r["flags"][k] = 1
        img, _ = osc.gather(oa.frame_params(**kw), W, H, gbuf, r)
        lit_ref = img[..., :3].sum(-1) > 0
        counts = osc.gather_counts(oa.frame_params(**kw), W, gbuf, r, np.arange(H))
        for cuts in (True, False):
            got, st = accum[cuts, k]
            lit = got[..., :3].sum(-1) > 0
            assert np.array_equal(lit, lit_ref), (cuts, k, np.argwhere(lit != lit_ref)[:8].tolist())
            assert (st["rays"], st["shaded"]) == counts, (cuts, k, st["rays"], st["shaded"], counts)
            assert st["rays"] == W * H
        assert accum[True, k][0].tobytes() == accum[False, k][0].tobytes(), k
        dark.append(int((~lit_ref).sum()))
    print("unlit pixels per VPL", dark)
    # every VPL above the grid throws shadows, none of them covers the image; the one below the grid throws none
    assert all(0 < d < W * H for d in dark[:-1]) and dark[-1] == 0, dark
