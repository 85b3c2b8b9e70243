"""Lightmap baking on the device (evplp_surface_points, evplp_lightmap_samples, evplp_bake_lightmap and their device forms).

  points   bytes against tests/lightmap_restate.py (float32 numpy, one rounding per operation, tex2d included) for synthetic hits on
           scenes.box_room textured and plain, every zeros case, both flags, n = 1, 63, 64, 65 and across the chunk boundary, host form =
           device form; and agreement with the renderer: the hits of evplp_trace_closest along eye -> g_pos give evplp_primary's texels.
  raster   triangle, beta and gamma bits against the int64 restatement for S = 1, 2, 4, one mesh and the whole scene, own texcoords and given
           uvs, overlapping charts, band boundaries, one triangle over the whole atlas, 5 000 triangles inside one tile.
  bake     against the oracle (restated points through evo_gather_vpl / evo_splat_photons with W = n, H = 1, resolved and gutter-filled in
           numpy) under the project's radiance bar, relative L2 <= 1e-5 per half; coverage and photons exact; bytes equal between band sizes
           and forms; the gutter; EVPLP_POINTS_WHITE; refusals; a refit that moves an occluder.

The renderer agreement leaves out the pixels whose traced hit lies on another triangle than the G-buffer's (edges and silhouettes: the ray
through g_pos is not the primary ray bit for bit) and fails above 2 % of the non-background, non-emitter pixels.  The oracle alone
(evo_primary against evo_closest_brute_batch on the same rays, seed 3, the room's camera, 64 x 64) leaves out 0.000 % (0 of 3 928 pixels).

Measured on an MI355X, 2026-10-21 (`pytest -s -m gpu tests/test_gpu_lightmap.py` prints them).  Renderer agreement: 0 of 3 928 pixels left out
on the plain and on the textured room, positions within 3.8e-7 / 2.0e-7 of the diagonal.  Bake, 48 x 48 at S = 2 (1 225 covered texels, 1 623
photon pairs): relative L2 against the 1e-5 bar 9.42e-8 for the VPL half and 1.57e-7 for the photon half; EVPLP_POINTS_WHITE 5.82e-8 / 1.36e-7;
the moved occluder changes 439 of 864 fully covered texels of the other charts, 8.56e-8 against the oracle of the moved scene."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lightmap_restate as lr
import oracle_api as oa
import scenes
from test_gpu_parity import REL_L2, rel_l2
from test_gpu_surface import inside32, planes_of

pytestmark = pytest.mark.gpu

F = np.float32
NPATHS, P = 64, 4
RES = 64
AGREE_CAP = 0.02


def say(*a):
    print("[lightmap]", *a, flush=True)


def room_scene(textured, n_boxes=3, tess=2, seed=3):
    """scenes.box_room with one more mesh at the end: a triangle without area (in no tree; its attributes are there)"""
    s = scenes.box_room(seed=seed, n_boxes=n_boxes, tess=tess, textured=textured)
    s.add_mesh([[1, 1, 1], [2, 2, 2], [3, 3, 3]], [(0, 1, 2)], 0)
    s.triangle_soup()
    return s


def mesh_first(sd, mesh):
    return int(sum(len(m["idx"]) for m in sd.meshes[:mesh]))


def context(evplp, sd, records=None):
    c = evplp.Context(RES, RES, NPATHS, NPATHS, P, deterministic=True)
    sd.upload(c)
    if records is not None:
        c.upload(evplp.BUF_RECORDS, records.astype(evplp.RECORD_DTYPE))
    return c


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class band:
    """EVPLP_LIGHTMAP_BAND for the calls inside"""

    def __init__(self, samples):
        self.samples = samples

    def __enter__(self):
        os.environ["EVPLP_LIGHTMAP_BAND"] = str(self.samples)

    def __exit__(self, *a):
        del os.environ["EVPLP_LIGHTMAP_BAND"]


# ---------------------------------------------------------------------------------------------------------------- points
def synthetic_hits(evplp, sd, n, seed):
    ntri = len(sd.triangle_soup()[0])
    rng = np.random.RandomState(seed)
    h = np.zeros(n, evplp.HIT_DTYPE)
    h["t"] = np.nan                                     # (never read)
    h["triangle"] = rng.randint(0, ntri, n)
    b = rng.rand(n).astype(F); g = (rng.rand(n).astype(F) * (F(1) - b)).astype(F)
    h["beta"], h["gamma"] = b, g
    corner = [(0, 0), (1, 0), (0, 1), (0.5, 0.5), (0.5, 0), (0, 0.25), (1.5, -0.25), (-0.0, 1.0)]      # corners, edges, outside the triangle
    for k in range(min(n, 64)):
        if k % 2 == 0:
            h["beta"][k], h["gamma"][k] = corner[(k // 2) % len(corner)]
    zeros = [(-1, 0.2, 0.2), (-2, 0.2, 0.2), (ntri, 0.2, 0.2), (ntri + 5, 0.1, 0.1), (2 ** 31 - 1, 0.1, 0.1), (-2 ** 31, 0.1, 0.1), (3, np.nan, 0.1), (3, 0.1, np.inf),
             (3, -np.inf, 0.1), (ntri - 1, 0.3, 0.3)]  # (the last: the triangle without area)
    if n >= 128:
        for k, (t, bb, gg) in enumerate(zeros):
            h["triangle"][65 + k], h["beta"][65 + k], h["gamma"][65 + k] = t, bb, gg
    return h, (np.arange(65, 65 + len(zeros)) if n >= 128 else np.arange(0))


@pytest.mark.parametrize("textured", (False, True))
def test_points_have_the_restatements_bytes(evplp, textured):
    import torch
    sd = room_scene(textured)
    big = evplp.QUERY_CHUNK_RAYS + 77
    hits, zeros = synthetic_hits(evplp, sd, big, 5)
    eyes = np.random.RandomState(6).uniform(-1.0, 11.0, (big, 3)).astype(F)
    with context(evplp, sd) as c:
        for flags in (0, evplp.POINTS_WHITE, evplp.POINTS_FACE_EYES, evplp.POINTS_WHITE | evplp.POINTS_FACE_EYES):
            want = lr.surface_points(sd, hits, flags, eyes)
            assert (want[zeros] == 0).all() and (bits(want[zeros]) == 0).all() and (want[:, 3] == 1).mean() > 0.99
            got = c.surface_points(hits, flags, eyes if flags & evplp.POINTS_FACE_EYES else None)
            assert got.dtype == evplp.SURFACE_POINT_DTYPE and np.array_equal(bits(got).reshape(-1, 16), bits(want)), \
                (textured, flags, np.argwhere(bits(got).reshape(-1, 16) != bits(want))[:6])
            if flags & evplp.POINTS_FACE_EYES:
                assert ((want[:, 4:7] * (eyes - want[:, 0:3])).sum(-1) >= -1e-3)[want[:, 3] == 1].all()
                plain = lr.surface_points(sd, hits, flags & 1)
                assert 0.02 < (bits(plain[:, 4:7]) != bits(want[:, 4:7])).any(-1).mean() < 0.98, "some normals flip, some do not"
            if flags & evplp.POINTS_WHITE:
                assert (got["rho_d"][got["valid"] == 1] == 1).all() and (got["rho_s"] == 0).all() and (got["phong_exp"] == 0).all()
            # the device form, and the sizes around a wave
            d = c.surface_points(torch.from_numpy(hits.view(np.int32).reshape(-1, 4)).cuda(), flags, torch.from_numpy(eyes).cuda() if flags & 2 else None)
            c.synchronize()
            assert np.array_equal(bits(d.cpu().numpy()), bits(want)), (textured, flags, "device form")
            for n in (1, 63, 64, 65):
                sub = c.surface_points(hits[:n], flags, eyes[:n] if flags & 2 else None)
                assert np.array_equal(bits(sub).reshape(-1, 16), bits(want[:n])), (n, flags)
        if textured:
            M = sd.triangle_soup()[2]
            inside = (hits["triangle"] >= 0) & (hits["triangle"] < len(M))
            floor = inside & (M[np.where(inside, hits["triangle"], 0)] == 5)
            plain = lr.surface_points(sd, hits, 0)
            assert len(np.unique(plain[floor & (plain[:, 3] == 1)][:, 8])) > 1000, "the floor's rho_d comes through the texture"
        assert c.surface_points(hits[:0]).shape == (0,)


def eye_rays(eye, pos, tmax):
    r = np.zeros((len(pos), 8), F)
    r[:, 0:3] = eye; r[:, 4:7] = pos - eye[None, :]; r[:, 7] = tmax
    return r


def agreement(sd, gbuf, hits_scene, hits_all, points):
    """the share of pixels left out, and the checks on the rest.  gbuf: four planes [n, 4]; hits_*: filter 1 and filter 0 along eye -> g_pos"""
    pos, nrm, dif, phg = gbuf
    soup = sd.triangle_soup()
    background = ~(nrm[:, :3] != 0).any(-1)
    emitter = (hits_all["triangle"] >= sd.light_first) & (hits_all["triangle"] < sd.light_first + sd.light_count)
    pool = ~background & ~emitter
    same = pool & (bits(points[:, 4:7]) == bits(nrm[:, :3])).all(-1) & (points[:, 3] == 1)
    diag = float(np.linalg.norm(soup[0].reshape(-1, 3).max(0) - soup[0].reshape(-1, 3).min(0)))
    err = np.abs(points[same, 0:3].astype(np.float64) - pos[same, :3]).max() if same.any() else 0.0
    assert err <= 1e-4 * diag, err
    return pool, same, err, diag


def test_points_of_traced_hits_agree_with_the_renderers_g_buffer(evplp, oracle):
    """left out when written: the oracle alone 0 of 3 928 pixels, the device 0 of 3 928 on either room (the cap is 2 %)"""
    sd = room_scene(False)
    eye = np.asarray(sd.cam_origin, F)
    # the oracle alone, before anything runs on the device: the cap must hold for this seed and camera without the product
    osc = oa.Scene(sd)
    og = [p.reshape(-1, 4) for p in osc.primary(RES, RES)[:4]]
    rays = eye_rays(eye, og[0][:, :3], F(1.5))
    oh1, oh0 = osc.closest_brute(rays, 1), osc.closest_brute(rays, 0)
    pool, same, err, diag = agreement(sd, og, oh1, oh0, lr.surface_points(sd, oh1))
    say(f"oracle alone: {int(pool.sum() - same.sum())} of {int(pool.sum())} pixels left out, position error {err / diag:.1e} of the diagonal")
    assert pool.sum() > 0.9 * RES * RES and (pool.sum() - same.sum()) <= AGREE_CAP * pool.sum()
    for textured in (False, True):
        sd = room_scene(textured)
        with context(evplp, sd) as c:
            c.primary((0.0, 0.0), clear_light=True)
            g = [c.download(b)[:RES].reshape(-1, 4) for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG)]
            rays = eye_rays(eye, g[0][:, :3], F(1.5))
            h1, h0 = c.trace_closest(rays, filter=1), c.trace_closest(rays, filter=0)
            pts = c.surface_points(h1).view(F).reshape(-1, 16)
        pool, same, err, diag = agreement(sd, g, h1, h0, pts)
        out = int(pool.sum() - same.sum())
        say(f"device, textured {textured}: {out} of {int(pool.sum())} pixels left out ({100.0 * out / pool.sum():.3f} %), position error {err / diag:.1e} of the diagonal")
        assert pool.sum() > 0.9 * RES * RES and out <= AGREE_CAP * pool.sum(), (out, int(pool.sum()))
        if not textured:
            assert np.array_equal(bits(pts[same, 8:11]), bits(g[2][same, :3])) and np.array_equal(bits(pts[same, 12:16]), bits(g[3][same]))
            assert (g[3][same, 3] > 0).any(), "glossy pixels among them"


# ---------------------------------------------------------------------------------------------------------------- raster
def packed_uvs(sd):
    """every mesh's chart in its own cell of a square grid, 80 % of the cell from its low corner: charts with empty texels between them, the
    first row and column touching the atlas border"""
    n = len(sd.meshes)
    side = int(math.ceil(math.sqrt(n)))
    out = []
    for k, m in enumerate(sd.meshes):
        o = np.array([k % side, k // side], F) / F(side)
        uv = (o[None, :] + m["uvs"] * F(0.8 / side)).astype(F)
        out.append(uv[m["idx"]].reshape(-1, 6))
    return np.ascontiguousarray(np.concatenate(out), F)


def same_hits(got, want):
    return np.array_equal(got["triangle"], want["triangle"]) and np.array_equal(bits(got["beta"]), bits(want["beta"])) and np.array_equal(bits(got["gamma"]), bits(want["gamma"])) \
        and (got["t"] == 0).all()


@pytest.fixture(scope="module")
def raster_room(evplp):
    sd = room_scene(True)
    c = context(evplp, sd)
    yield sd, c
    c.close() if hasattr(c, "close") else c.__exit__(None, None, None)


@pytest.mark.parametrize("S", (1, 2, 4))
def test_raster_equals_the_int64_restatement(evplp, raster_room, S):
    sd, c = raster_room
    U = sd.triangle_soup()[1]
    # the whole scene with its own texcoords: every quad's chart is [0, 1]^2, so they all overlap and the lowest index wins
    W, H = 24, 20
    want = lr.rasterise(U, 0, W, H, S, evplp.HIT_DTYPE)
    got = c.lightmap_samples(W, H, S)
    assert same_hits(got, want), np.argwhere(got["triangle"] != want["triangle"])[:6]
    assert (want["triangle"] >= 0).all() and want["triangle"].max() < len(sd.meshes[0]["idx"]), "mesh 0 covers the atlas and wins everywhere"
    # one mesh, own texcoords
    mesh = 7
    first, count = mesh_first(sd, mesh), len(sd.meshes[mesh]["idx"])
    want = lr.rasterise(U[first:first + count], first, W, H, S, evplp.HIT_DTYPE)
    assert same_hits(c.lightmap_samples(W, H, S, mesh=mesh), want) and want["triangle"].min() >= first
    # given uvs: the packed atlas (charts apart, empty texels between), in one band and in bands of one and of a few rows, and the device form
    W = H = 61
    uv = packed_uvs(sd)
    want = lr.rasterise(uv, 0, W, H, S, evplp.HIT_DTYPE)
    assert 0.3 < (want["triangle"] >= 0).mean() < 0.8 and len(np.unique(want["triangle"])) > len(sd.meshes)
    got = c.lightmap_samples(W, H, S, uvs=uv)
    assert same_hits(got, want), np.argwhere(got["triangle"] != want["triangle"])[:6]
    for samples in (1, 5 * W * S * S + 3):
        with band(samples):
            assert c.lightmap_samples(W, H, S, uvs=uv).tobytes() == got.tobytes(), samples
    with band(9 * W * S * S):
        d = c.lightmap_samples_device(W, H, S, uvs=uv)
        c.synchronize()
        assert d.cpu().numpy().tobytes() == got.tobytes()
    # random uvs: mirrored charts, charts reaching outside [0, 1]^2 (clipped, not wrapped), overlap everywhere
    rng = np.random.RandomState(20 + S)
    count = len(sd.meshes[9]["idx"]); first = mesh_first(sd, 9)
    uv = rng.uniform(-0.3, 1.3, (count, 6)).astype(F)
    uv[1] = [0.1, 0.1, 0.5, 0.5, 0.9, 0.9]; uv[2, 3] = np.nan; uv[3, 0] = np.inf; uv[4, 5] = 3.0e38       # no area, and three that do not snap
    want = lr.rasterise(uv, first, 33, 17, S, evplp.HIT_DTYPE)
    assert same_hits(c.lightmap_samples(33, 17, S, mesh=9, uvs=uv), want)
    assert not np.isin(want["triangle"], first + np.arange(1, 5)).any()
    # one triangle over the whole atlas (the light mesh's first; the others do not snap, or lose to it)
    lm = sd.light_mesh
    count = len(sd.meshes[lm]["idx"]); first = mesh_first(sd, lm)
    uv = np.full((count, 6), np.nan, F); uv[0] = [-1, -1, 3, -1, -1, 3]; uv[1] = [-1, -1, -1, 3, 3, -1]
    got = c.lightmap_samples(64, 64, S, mesh=lm, uvs=uv)
    assert same_hits(got, lr.rasterise(uv, first, 64, 64, S, evplp.HIT_DTYPE)) and (got["triangle"] == first).all()


def test_raster_with_five_thousand_triangles_inside_one_tile(evplp):
    sd = scenes.box_room(seed=2, n_boxes=8, tess=6)
    ntri = len(sd.triangle_soup()[0])
    assert ntri >= 5000
    rng = np.random.RandomState(9)
    W = H = 32
    # every triangle inside tile (1, 2) of the 32 x 32 atlas: texels 8 .. 16 by 16 .. 24
    c0 = np.array([8.0 / W, 16.0 / H])
    uv = (c0[None, None, :] + rng.uniform(0.0, 8.0 / W, (ntri, 3, 2))).astype(F).reshape(ntri, 6)
    want = lr.rasterise(uv, 0, W, H, 2, evplp.HIT_DTYPE)
    with context(evplp, sd) as c:
        got = c.lightmap_samples(W, H, 2, uvs=uv)
        with band(W * 4 * 3):
            again = c.lightmap_samples(W, H, 2, uvs=uv)
    inside = np.zeros((H, W), bool); inside[16:24, 8:16] = True
    assert (want["triangle"][~inside] == -1).all() and (want["triangle"][inside] >= 0).mean() > 0.99
    assert same_hits(got, want) and again.tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------------------- bake
class Bake:
    """the scene, the oracle's records, the packed atlas at S = 2 and per sample the oracle's two estimates -- computed once"""
    W = H = 48
    S = 2
    MODE = 1

    def __init__(self, evplp):
        self.sd = room_scene(False)
        self.osc = oa.Scene(self.sd)
        self.records = self.osc.trace_light_paths(7, NPATHS, P)
        self.uv = packed_uvs(self.sd)
        self.radius = 0.6
        self.hits = lr.rasterise(self.uv, 0, self.W, self.H, self.S, evplp.HIT_DTYPE)
        self.ref = self.reference(evplp, 0)

    def params(self, **kw):
        p = dict(camera_pos=self.sd.cam_origin, mis_mode=self.MODE, pdf_mc=1.0 / (np.pi * self.radius ** 2), clamping_value=0.05, photon_radius=self.radius,
                 num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P)
        p.update(kw)
        return p

    def reference(self, evplp, flags, osc=None, sd=None):
        """the texels before the gutter, from the restated points through the oracle"""
        shape = self.hits.shape
        pts = lr.surface_points(sd or self.sd, self.hits.reshape(-1), flags)
        valid = pts[:, 3] == 1
        sub = np.ascontiguousarray(pts[valid]).view(evplp.SURFACE_POINT_DTYPE).reshape(-1)
        fp = oa.frame_params(**self.params())
        g = planes_of(sub)
        vpl_s, _ = (osc or self.osc).gather(fp, len(sub), 1, g, self.records)
        pm_s, pairs = oa.splat(fp, len(sub), 1, g, self.records)
        usable = (self.records["flags"] & 2) != 0
        usable[0] = False
        count_s = inside32(self.records["pos"][usable], sub["pos"], self.radius).sum(0)
        assert int(count_s.sum()) == pairs, (int(count_s.sum()), pairs)
        vpl = np.zeros((len(pts), 3), F); pm = np.zeros((len(pts), 3), F); ph = np.zeros(len(pts), F)
        vpl[valid] = vpl_s[0, :, :3]; pm[valid] = pm_s[0, :, :3]; ph[valid] = count_s
        self.pairs = pairs
        return lr.resolve(valid.reshape(shape), vpl.reshape(shape + (3,)), pm.reshape(shape + (3,)), ph.reshape(shape), evplp.LIGHTMAP_TEXEL_DTYPE)


@pytest.fixture(scope="module")
def bake(evplp, oracle):
    b = Bake(evplp)
    assert (b.records["flags"] & 1).sum() > 40 and (b.records["flags"] & 2).sum() > 40
    cov = b.ref["coverage"]
    assert 0.3 < (cov > 0).mean() < 0.8 and ((cov > 0) & (cov < 1)).sum() > 50, "covered, empty and partly covered texels"
    assert b.pairs > 1000 and np.abs(b.ref["vpl"]).max() > 1e-3 and np.abs(b.ref["pm"]).max() > 1e-5
    with context(evplp, b.sd, b.records) as c:
        b.got = {g: c.bake_lightmap(evplp.frame_params(**b.params()), b.W, b.H, b.S, gutter=g, uvs=b.uv) for g in (0, 1, 3)}
    return b


def test_bake_against_the_oracle(evplp, bake):
    got, ref = bake.got[0], bake.ref
    assert np.array_equal(bits(got["coverage"]), bits(ref["coverage"])), "coverage is exact"
    assert np.array_equal(bits(got["photons"]), bits(ref["photons"])), "the mean pair count is exact"
    assert (bits(got.view(F).reshape(bake.H, bake.W, 8)[ref["coverage"] == 0]) == 0).all(), "an uncovered texel is 32 zero bytes"
    say(f"bake {bake.W} x {bake.H} at S = {bake.S}: VPL rel L2 {rel_l2(got['vpl'], ref['vpl']):.2e}, photons rel L2 {rel_l2(got['pm'], ref['pm']):.2e} (bar {REL_L2}); "
        f"{bake.pairs} photon pairs, {int((ref['coverage'] > 0).sum())} covered texels")
    assert rel_l2(got["vpl"], ref["vpl"]) <= REL_L2 and rel_l2(got["pm"], ref["pm"]) <= REL_L2
    for g in (1, 3):
        want = lr.gutter(ref, g)
        assert np.array_equal(bits(bake.got[g]["coverage"]), bits(want["coverage"])) and np.array_equal(bits(bake.got[g]["photons"]), bits(want["photons"])), g
        assert rel_l2(bake.got[g]["vpl"], want["vpl"]) <= REL_L2 and rel_l2(bake.got[g]["pm"], want["pm"]) <= REL_L2, g


def test_gutter_passes(evplp, bake):
    base = bake.got[0]
    cov = base["coverage"]
    for g in (1, 3):
        got = bake.got[g]
        assert got.tobytes() == lr.gutter(base, g).tobytes(), g
        assert got[cov != 0].tobytes() == base[cov != 0].tobytes(), "a covered texel is not touched"
        assert set(np.unique(got["coverage"][cov == 0]).tolist()) == set([0.0] + [-float(d) for d in range(1, g + 1)]), np.unique(got["coverage"][cov == 0])
    edge = np.zeros(cov.shape, bool); edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
    assert (bake.got[3]["coverage"][edge] < 0).sum() > 10 and (cov[edge] > 0).sum() > 10, "filled and covered texels on the atlas border"


def test_bake_bytes_do_not_depend_on_the_band_or_the_form(evplp, bake):
    fp = evplp.frame_params(**bake.params())
    per_row = bake.W * bake.S * bake.S
    with context(evplp, bake.sd, bake.records) as c:
        for samples, g in ((1, 0), (7 * per_row + 1, 3), (25 * per_row, 1)):
            with band(samples):
                assert c.bake_lightmap(fp, bake.W, bake.H, bake.S, gutter=g, uvs=bake.uv).tobytes() == bake.got[g].tobytes(), samples
        for g in (0, 1, 3):
            with band(11 * per_row):
                d = c.bake_lightmap_device(fp, bake.W, bake.H, bake.S, gutter=g, uvs=bake.uv)
            c.synchronize()
            assert d.cpu().numpy().tobytes() == bake.got[g].tobytes(), g
        # one half at a time: the other half's floats are zero, the rest the same bytes
        v = c.bake_lightmap(fp, bake.W, bake.H, bake.S, uvs=bake.uv, what=evplp.SURFACE_VPL)
        assert np.array_equal(bits(v["vpl"]), bits(bake.got[0]["vpl"])) and (v["pm"] == 0).all() and (v["photons"] == 0).all() and np.array_equal(v["coverage"], bake.got[0]["coverage"])
        # the samples are the rasteriser's, the points evplp_surface_points', the light evplp_gather_surface's
        hits = c.lightmap_samples(bake.W, bake.H, bake.S, uvs=bake.uv)
        light = c.gather_surface(c.surface_points(hits.reshape(-1)), fp)
        shape = hits.shape
        mine = lr.resolve((hits["triangle"] >= 0), light["vpl"].reshape(shape + (3,)), light["pm"].reshape(shape + (3,)), light["photons"].reshape(shape), evplp.LIGHTMAP_TEXEL_DTYPE)
        assert mine.tobytes() == bake.got[0].tobytes()


def test_white_points_give_the_irradiance(evplp, bake):
    fp = evplp.frame_params(**bake.params())
    with context(evplp, bake.sd, bake.records) as c:
        got = c.bake_lightmap(fp, bake.W, bake.H, bake.S, flags=evplp.POINTS_WHITE, uvs=bake.uv)
    ref = bake.reference(evplp, evplp.POINTS_WHITE)            # the oracle's radiance with rho_d = 1, rho_s = 0: E / pi
    e_got, e_ref = got["vpl"].astype(np.float64) * np.pi, ref["vpl"].astype(np.float64) * np.pi
    say(f"white bake: irradiance rel L2 {rel_l2(e_got, e_ref):.2e}, photons {rel_l2(got['pm'], ref['pm']):.2e}")
    assert rel_l2(e_got, e_ref) <= REL_L2 and rel_l2(got["pm"], ref["pm"]) <= REL_L2
    assert np.array_equal(got["coverage"], bake.got[0]["coverage"]) and not np.array_equal(got["vpl"], bake.got[0]["vpl"])


def test_refusals_leave_the_output_untouched_and_the_context_usable(evplp, bake):
    import torch
    L = evplp.lib()
    INV = evplp.ERR_INVALID
    BOTH = evplp.SURFACE_VPL | evplp.SURFACE_PHOTONS
    W, H, S = bake.W, bake.H, bake.S
    out = np.full(W * H * 32, 0x5A, np.uint8)
    hits = np.zeros(8, evplp.HIT_DTYPE); pts = np.full(8 * 64, 0x5A, np.uint8); samples = np.full(W * H * S * S * 16, 0x5A, np.uint8)
    uv = bake.uv
    op, up, hp, pp, sp = out.ctypes.data, uv.ctypes.data, hits.ctypes.data, pts.ctypes.data, samples.ctypes.data

    def fpr(**kw):
        return C.byref(evplp.frame_params(**bake.params(**kw)))

    def prm(**kw):
        d = dict(mesh=-1, width=W, height=H, samples=S, gutter=1, flags=0); d.update(kw)
        return C.byref(evplp.LightmapParams(d["mesh"], d["width"], d["height"], d["samples"], d["gutter"], d["flags"]))
    with evplp.Context(RES, RES, NPATHS, NPATHS, P, deterministic=True) as c:           # no evplp_build_accel yet
        assert L.evplp_bake_lightmap(c._h, fpr(), BOTH, prm(), up, op) == INV and b"evplp_build_accel" in L.evplp_last_error(c._h)
        assert L.evplp_lightmap_samples(c._h, -1, up, W, H, S, sp) == INV and L.evplp_surface_points(c._h, hp, 8, 0, None, pp) == INV
        bake.sd.upload(c)
        c.upload(evplp.BUF_RECORDS, bake.records.astype(evplp.RECORD_DTYPE))
        for form in (L.evplp_bake_lightmap, L.evplp_bake_lightmap_device):
            assert form(c._h, fpr(), BOTH, None, up, op) == INV and form(c._h, fpr(), BOTH, prm(), up, None) == INV and form(c._h, None, BOTH, prm(), up, op) == INV
            for bad in (dict(mesh=-2), dict(mesh=len(bake.sd.meshes)), dict(width=0), dict(width=8193), dict(height=0), dict(height=8193), dict(samples=0), dict(samples=3),
                        dict(samples=8), dict(gutter=-1), dict(gutter=9), dict(flags=2), dict(flags=4)):
                assert form(c._h, fpr(), BOTH, prm(**bad), up, op) == INV, bad
            # everything evplp_gather_surface refuses
            assert form(c._h, fpr(), 0, prm(), up, op) == INV and form(c._h, fpr(), 4, prm(), up, op) == INV
            assert form(c._h, fpr(mis_mode=6), BOTH, prm(), up, op) == INV
            for r in (0.0, -1.0, float("nan"), float("inf")):
                assert form(c._h, fpr(photon_radius=r), BOTH, prm(), up, op) == INV, r
            for bad in (dict(num_vpl_light_paths=0), dict(photons_per_path=0), dict(num_light_paths=0), dict(num_vpl_light_paths=NPATHS + 1), dict(num_light_paths=NPATHS + 1),
                        dict(photons_per_path=P + 1)):
                assert form(c._h, fpr(**bad), BOTH, prm(), up, op) == INV, bad
        for form in (L.evplp_lightmap_samples, L.evplp_lightmap_samples_device):
            for bad in ((-2, W, H, S), (len(bake.sd.meshes), W, H, S), (-1, 0, H, S), (-1, W, 8193, S), (-1, W, H, 3)):
                assert form(c._h, bad[0], up, bad[1], bad[2], bad[3], sp) == INV, bad
            assert form(c._h, -1, up, W, H, S, None) == INV
        for form in (L.evplp_surface_points, L.evplp_surface_points_device):
            assert form(c._h, hp, -1, 0, None, pp) == INV and form(c._h, None, 8, 0, None, pp) == INV and form(c._h, hp, 8, 0, None, None) == INV
            assert form(c._h, hp, 8, 4, None, pp) == INV and form(c._h, hp, 8, evplp.POINTS_FACE_EYES, None, pp) == INV and b"eyes" in L.evplp_last_error(c._h)
            assert form(c._h, hp, 0, 0, None, pp) == evplp.OK and form(c._h, None, 0, 0, None, None) == evplp.OK
        assert (out == 0x5A).all() and (pts == 0x5A).all() and (samples == 0x5A).all(), "a refused call writes nothing"
        # the device forms' destinations must be 16-byte aligned
        o = torch.full((W * H * 8 + 4,), 7.0, dtype=torch.float32, device="cuda")
        assert L.evplp_bake_lightmap_device(c._h, fpr(), BOTH, prm(), None, C.c_void_p(o.data_ptr() + 4)) == INV and b"aligned" in L.evplp_last_error(c._h)
        assert L.evplp_lightmap_samples_device(c._h, -1, None, 8, 8, 1, C.c_void_p(o.data_ptr() + 4)) == INV
        c.synchronize()
        assert (o.cpu().numpy() == 7.0).all()
        # a radius that is not used is not looked at; and the context is usable afterwards
        fp = evplp.frame_params(**bake.params())
        assert c.bake_lightmap(fp, W, H, S, gutter=1, uvs=uv).tobytes() == bake.got[1].tobytes()
        v = c.bake_lightmap(evplp.frame_params(**bake.params(photon_radius=0.0)), W, H, S, uvs=uv, what=evplp.SURFACE_VPL)
        assert np.array_equal(bits(v["vpl"]), bits(bake.got[0]["vpl"]))
        # dirty vertices: refused until the refit
        c.transform_mesh(6 + 5, [1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, 1, 0])
        assert L.evplp_bake_lightmap(c._h, fpr(), BOTH, prm(), up, op) == INV and b"evplp_refit_accel" in L.evplp_last_error(c._h)
        assert L.evplp_lightmap_samples(c._h, -1, up, W, H, S, sp) == INV and L.evplp_surface_points(c._h, hp, 8, 0, None, pp) == INV
        assert (out == 0x5A).all() and (pts == 0x5A).all() and (samples == 0x5A).all()


def test_a_refit_that_moves_an_occluder_changes_the_texels_behind_it(evplp, bake):
    mesh = 6 + 5                                    # the top face of the first box: doubled and lifted under the light
    centre = bake.sd.meshes[mesh]["verts"].mean(0)
    s = 2.0
    t = np.array([4.2, 3.9, 3.6]) - s * centre
    fp = evplp.frame_params(**bake.params())
    with context(evplp, bake.sd, bake.records) as c:
        c.transform_mesh(mesh, [s, 0, 0, t[0], 0, s, 0, t[1], 0, 0, s, t[2]])
        with pytest.raises(evplp.EvplpError) as e:
            c.bake_lightmap(fp, bake.W, bake.H, bake.S, uvs=bake.uv)
        assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value)
        c.refit_accel()
        got = c.bake_lightmap(fp, bake.W, bake.H, bake.S, uvs=bake.uv, what=evplp.SURFACE_VPL)
        now = scenes.moved(bake.sd)
        now.meshes[mesh]["verts"] = c.mesh_vertices(mesh, 0)
        now.triangle_soup()
    ref = bake.reference(evplp, 0, oa.Scene(now), now)
    base = bake.got[0]
    assert np.array_equal(got["coverage"], base["coverage"]), "the atlas is the same: the chart did not move"
    owner = bake.hits["triangle"][:, :, 0, 0]
    first, count = mesh_first(bake.sd, mesh), len(bake.sd.meshes[mesh]["idx"])
    elsewhere = (base["coverage"] == 1) & ~((owner >= first) & (owner < first + count))
    changed = elsewhere & (got["vpl"] != base["vpl"]).any(-1)
    say(f"moved occluder: {int(changed.sum())} of {int(elsewhere.sum())} fully covered texels of other charts changed; VPL rel L2 against the oracle {rel_l2(got['vpl'], ref['vpl']):.2e}")
    assert changed.sum() > 50
    assert rel_l2(got["vpl"], ref["vpl"]) <= REL_L2
