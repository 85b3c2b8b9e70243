"""The surface gather on the device (evplp_gather_surface, its device form): the renderer's two estimates at a caller's surface points.

  1, 2  the material domain (tests/shading_domain.py): the 44 x 28 floor receiver as 1 232 points, per record and per mode against the
        float64 restatement under the project's K (K_GPU_GATHER = 8, K_GPU_SPLAT = 18 of test_gpu_shading_domain.py), and the whole set.
  3     scenes.box_room, records traced by the oracle (2 000 x 4 slots; the VPL half reads the first 160 x 4), the points the oracle's own
        64 x 48 G-buffer: evo_gather_vpl and evo_splat_photons with W = n, H = 1 are the references, under the project's bars (image
        relative L2 1e-5, per point 2e-4: test_gpu_parity.assert_image_close); lit per point against evo_occluded_brute on the pairs that
        pass the float32 cosine test and against evplp_trace_occluded; sum(photons) against the oracle's pairs.
  4     eyes; 5 a point's bytes; 6 a hostile grid; 7 edges and refusals; 8 a moved occluder; 9 agreement with the frame's own passes.

Measured on an MI355X, 2026-10-21 (`pytest -s -m gpu tests/test_gpu_surface.py` prints them), error / bar at its worst.  Material domain,
VPL half (K = 8): per record 0.402 / 0.369 / 0.369 / 0.370 / 0.402 / 0.402 in modes 0 - 5, the whole set 0.394 / 0.362 / 0.362 / 0.363 /
0.394 / 0.394; photon half (K = 18): 0.180 / 0.148 / 0.147 / 0.148 / 0.147 / 0.453.  Room (3 072 points, 1 043 337 shadow rays of which
942 889 lit, 6 629 photon pairs; the oracle's tree and its brute force agree on every ray): relative L2 against the 1e-5 bar 2.81e-7 /
2.89e-7 / 2.81e-7 for the VPL half and 1.07e-7 / 4.09e-7 / 6.20e-7 for the photon half in modes 0, 1, 5.  The frame's own passes: 3.07e-7
against gather_lvc, 5.24e-7 against splat_photons, under twice the bars.  The moved occluder changes the lit count of 2 864 points.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_api as oa
import scenes
import shading_domain as sd
from test_gpu_parity import REL_L2, PIX_REL, assert_image_close, rel_l2
from test_gpu_shading_domain import K_GPU_GATHER, K_GPU_SPLAT, MODES, compare, dom  # noqa: F401  (dom: the module's fixture)

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48
NPATHS, NVPL, P = 2000, 160, 4
TMIN, TMAX = F(0.0001), F(1.0) - F(0.0001)
ROOM_MODES = (0, 1, 5)


def say(*a):
    print("[surface]", *a, flush=True)


def points_of(evplp, gbuf):
    """the four planes of a G-buffer ([..., 4] each) as SURFACE_POINT_DTYPE, flattened"""
    n = gbuf[0].reshape(-1, 4).shape[0]
    pts = np.zeros(n, evplp.SURFACE_POINT_DTYPE)
    flat = pts.view(F).reshape(n, 16)
    for k in range(4):
        flat[:, 4 * k:4 * k + 4] = gbuf[k].reshape(-1, 4)
    return pts


def planes_of(pts):
    """back: the oracle's G-buffer arrays of W = n, H = 1"""
    flat = np.ascontiguousarray(pts).view(F).reshape(-1, 16)
    return [np.ascontiguousarray(flat[:, 4 * k:4 * k + 4]).reshape(1, -1, 4) for k in range(4)]


def dot32(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z, every operation rounded to float32 on its own (dot_exact)"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def inside32(photon_pos, X, r):
    """evo_photon_frag's test in float32: [photons, points]"""
    dv = photon_pos[:, None, :].astype(F) - X[None, :, :].astype(F)
    return ~(dot32(dv, dv) > F(r) * F(r))


# ---------------------------------------------------------------------------------------------------------------- 1, 2: the material domain
def domain_context(evplp, dom, paths=sd.NPATHS, per=sd.P):
    c = evplp.Context(sd.W, sd.H, paths, paths, per, bvh_builder=evplp.BVH_SAH, deterministic=True)
    dom.scene.upload(c)
    return c


@pytest.mark.parametrize("mode", MODES)
def test_vpl_half_per_record_over_the_material_domain(evplp, dom, mode):
    """worst error / bar per record 0.402 / 0.369 / 0.369 / 0.370 / 0.402 / 0.402 in modes 0 - 5 at K = 8 (MI355X, 2026-10-21)"""
    pts = points_of(evplp, dom.gbuf)
    fp = evplp.frame_params(**sd.params(mode))
    worst = 0.0
    with domain_context(evplp, dom) as c:
        for k, name in enumerate(dom.vpl_names):
            c.upload(evplp.BUF_RECORDS, sd.only_slot(dom.vpls, k, 1))
            got = c.gather_surface(pts, fp, what=evplp.SURFACE_VPL).reshape(sd.H, sd.W)
            val, kappa, lam, decided, lit = dom.vpl_ref(mode, k)
            what = f"surface VPL half mode {mode} record {name}"
            assert int(got["lit"].sum()) == dom.counts[k][1] and (got["lit"] >= 0).all(), (what, got["lit"].sum(), dom.counts[k])
            assert np.all(got["lit"][~lit] == 0) and np.all(got["vpl"][~lit] == 0.0), what + ": an unlit pair contributes"
            assert np.all(got.view(F).reshape(sd.H, sd.W, 8)[~dom.pixel.stencil] == 0.0), what + ": a stencilled-out point was written"
            assert np.all(got["pm"] == 0.0) and np.all(got["photons"] == 0.0), what + ": the half not asked for"
            if name in sd.DARK_VPLS:
                assert np.all(got["vpl"] == 0.0), what
            worst = max(worst, compare(got["vpl"] * F(sd.NPATHS), (val, kappa, lam, decided), K_GPU_GATHER, what))
        # the whole set, against the summed bars (test_gather_whole_set forms them)
        n = len(dom.vpl_names)
        refs = [dom.vpl_ref(mode, k) for k in range(n)]
        total = sum(r[0] for r in refs)
        bars = sum(sd.bar(r[0], r[1], r[2], K_GPU_GATHER, True) for r in refs) + n * 2.0 ** -24 * sum(np.abs(r[0]) for r in refs)
        decided = np.logical_and.reduce([r[3] for r in refs])
        c.upload(evplp.BUF_RECORDS, dom.vpls)
        got = c.gather_surface(pts, fp, what=evplp.SURFACE_VPL).reshape(sd.H, sd.W)
    assert int(got["lit"].sum()) == sum(s for _, s in dom.counts)
    assert np.array_equal(got["lit"], sum(r[4] for r in refs).astype(F)), "nothing occludes on the floor: lit = the pairs that pass the cosine test"
    ratio = np.where(decided[..., None], np.abs(got["vpl"].astype(np.float64) * sd.NPATHS - total) / bars, 0.0)
    say(f"VPL half, material domain, mode {mode}: per record worst error / bar {worst:.3f} (K = {K_GPU_GATHER}); whole set {float(ratio.max()):.3f}")
    assert ratio.max() <= 1.0, (mode, np.unravel_index(int(ratio.argmax()), ratio.shape), float(ratio.max()))


@pytest.mark.parametrize("mode", MODES)
def test_photon_half_per_photon_over_the_material_domain(evplp, dom, mode):
    """worst error / bar 0.180 / 0.148 / 0.147 / 0.148 / 0.147 / 0.453 in modes 0 - 5 at K = 18 (MI355X, 2026-10-21)"""
    pts = points_of(evplp, dom.gbuf)
    fp = evplp.frame_params(**sd.params(mode))
    stencil = dom.pixel.stencil
    worst = 0.0
    with domain_context(evplp, dom) as c:
        for k, (name, s) in enumerate(zip(dom.photon_names, dom.photon_slots)):
            c.upload(evplp.BUF_RECORDS, sd.only_slot(dom.photons, s, 2))
            got = c.gather_surface(pts, fp, what=evplp.SURFACE_PHOTONS).reshape(sd.H, sd.W)
            val, kappa, lam, decided, inside, rdec = dom.photon_ref(mode, k)
            what = f"surface photon half mode {mode} photon {name}"
            assert rdec.all(), what
            assert np.array_equal(got["photons"], (inside & stencil).astype(F)), (what, int(got["photons"].sum()), int((inside & stencil).sum()))
            assert np.all(got["pm"][~inside] == 0.0), what + ": a point outside the radius was written"
            assert np.all(got.view(F).reshape(sd.H, sd.W, 8)[~stencil] == 0.0) and np.all(got["vpl"] == 0.0) and np.all(got["lit"] == 0.0), what
            worst = max(worst, compare(got["pm"], (val, kappa, lam, decided & stencil), K_GPU_SPLAT, what))
    say(f"photon half, material domain, mode {mode}: worst error / bar {worst:.3f} (K = {K_GPU_SPLAT})")


# ---------------------------------------------------------------------------------------------------------------- 3: the room
class Room:
    """the scene, the oracle's records and G-buffer, and every (usable VPL slot, point) pair that passes the float32 cosine test with its
    shadow ray and the oracle's two answers -- computed once"""

    def __init__(self, evplp):
        self.scene = scenes.box_room(seed=3, n_boxes=6, tess=2, aspect=W / H)
        self.osc = oa.Scene(self.scene)
        self.records = self.osc.trace_light_paths(5, NPATHS, P)
        self.gbuf = self.osc.primary(W, H)[:4]
        self.pts = points_of(evplp, self.gbuf)
        self.n = len(self.pts)
        self.radius = float(F(0.03 * 0.5 * np.sqrt(10.0 ** 2 + 8.0 ** 2 + 5.0 ** 2)))
        self.valid = self.pts["valid"] != 0
        self.set_pairs(np.arange(self.n))

    def params(self, mode, eye=None):
        return dict(camera_pos=self.scene.cam_origin if eye is None else eye, mis_mode=mode, pdf_mc=1.0 / (np.pi * self.radius ** 2), clamping_value=0.05,
                    photon_radius=self.radius, num_light_paths=NPATHS, num_vpl_light_paths=NVPL, photons_per_path=P)

    def set_pairs(self, idx):
        rec, X, N = self.records, self.pts["pos"][idx], self.pts["normal"][idx]
        ok = self.valid[idx]
        rays, where = [], []
        for k in np.nonzero(rec["flags"][:NVPL * P] & 1)[0]:
            v12 = rec["pos"][k][None, :] - X
            c1 = np.maximum(dot32(N, v12), F(0)); c2 = np.maximum(-dot32(np.broadcast_to(rec["normal"][k], v12.shape), v12), F(0))
            j = np.nonzero(ok & (c1 * c2 > 0))[0]
            r = np.zeros((len(j), 8), F)
            r[:, 0:3] = rec["pos"][k]; r[:, 3] = TMIN; r[:, 4:7] = -v12[j]; r[:, 7] = TMAX
            rays.append(r); where.append(idx[j])
        self.rays = np.concatenate(rays); self.where = np.concatenate(where); self.idx = idx

    def brute_lit(self, osc=None):
        occ = (osc or self.osc).occluded_brute(self.rays)
        lit = np.zeros(self.n, np.int64)
        np.add.at(lit, self.where[occ == 0], 1)
        return lit, occ

    def tree_occluded(self):
        out = np.zeros(len(self.rays), np.uint8)
        base = self.rays.ctypes.data
        fn, h = self.osc.lib.evo_occluded, self.osc.h
        for i in range(len(self.rays)):
            out[i] = fn(h, C.c_void_p(base + 32 * i), C.c_void_p(base + 32 * i + 16), C.c_float(TMIN), C.c_float(TMAX))
        return out

    def oracle(self, mode, pts=None, eye=None):
        """(vpl [n, 3], pm [n, 3], pairs) of evo_gather_vpl and evo_splat_photons with W = n, H = 1"""
        pts = self.pts if pts is None else pts
        g = planes_of(pts)
        fp = oa.frame_params(**self.params(mode, eye))
        vpl, _ = self.osc.gather(fp, len(pts), 1, g, self.records)
        pm, pairs = oa.splat(fp, len(pts), 1, g, self.records)
        return vpl[0, :, :3], pm[0, :, :3], pairs


@pytest.fixture(scope="module")
def room(evplp, oracle):
    r = Room(evplp)
    usable = r.records["flags"]
    assert (usable[:NVPL * P] & 1).sum() > 200 and (usable & 2).sum() > 2000 and r.valid.sum() > 0.9 * r.n
    r.lit, r.occ = r.brute_lit()
    aside = r.tree_occluded() != r.occ
    assert aside.sum() <= 0.005 * len(r.rays)
    assert aside.sum() == 0, "with these seeds evo_occluded and evo_occluded_brute agree on every shadow ray"
    say(f"room: {r.n} points, {len(r.rays)} shadow rays, {int(r.lit.sum())} lit pairs")
    assert 0.2 < r.lit.sum() / len(r.rays) < 0.95, "occluded and lit pairs both"
    r.refs = {mode: r.oracle(mode) for mode in ROOM_MODES}
    return r


def room_context(evplp, room, records=None):
    c = evplp.Context(W, H, NPATHS, NVPL, P, deterministic=True)
    room.scene.upload(c)
    c.upload(evplp.BUF_RECORDS, (room.records if records is None else records).astype(evplp.RECORD_DTYPE))
    return c


@pytest.fixture(scope="module")
def base(evplp, room):
    """both halves of every point in the three modes: what every other form is compared with, byte for byte"""
    with room_context(evplp, room) as c:
        return {mode: c.gather_surface(room.pts, evplp.frame_params(**room.params(mode))) for mode in ROOM_MODES}


@pytest.mark.parametrize("mode", ROOM_MODES)
def test_room_both_halves_against_the_oracle(room, base, mode):
    """relative L2, VPL half 2.81e-7 / 2.89e-7 / 2.81e-7, photon half 1.07e-7 / 4.09e-7 / 6.20e-7 in modes 0, 1, 5 (MI355X, 2026-10-21)"""
    got = base[mode]
    vpl, pm, pairs = room.refs[mode]
    assert np.array_equal(got["lit"], np.where(room.valid, room.lit, 0).astype(F)), np.nonzero(got["lit"] != room.lit)[0][:8]
    assert int(got["photons"].sum()) == pairs and pairs > 5000, (got["photons"].sum(), pairs)
    assert (got["photons"] > 0).mean() > 0.3 and np.abs(vpl).max() > 1e-3 and np.abs(pm).max() > 1e-4
    say(f"room mode {mode}: VPL rel L2 {rel_l2(got['vpl'], vpl):.2e}, photons rel L2 {rel_l2(got['pm'], pm):.2e} (bar {REL_L2}); {pairs} photon pairs")
    assert_image_close(got["vpl"], vpl, what=f"VPL half mode {mode}")
    assert_image_close(got["pm"], pm, what=f"photon half mode {mode}")


def test_lit_equals_the_occlusion_query(evplp, room, base):
    with room_context(evplp, room) as c:
        occ = c.trace_occluded(room.rays)
    assert np.array_equal(occ, room.occ), "evplp_trace_occluded answers these rays as evo_occluded_brute does"
    per = np.zeros(room.n, np.int64)
    np.add.at(per, room.where[occ == 0], 1)
    for mode in ROOM_MODES:
        assert np.array_equal(base[mode]["lit"], per.astype(F))


# ---------------------------------------------------------------------------------------------------------------- 4: eyes
def test_eyes(evplp, room, base):
    mode = 1
    fp = evplp.frame_params(**room.params(mode))
    cam = np.asarray(room.scene.cam_origin, F)
    eyes4 = np.array([cam, [2.0, 1.5, 4.0], [8.5, 6.0, 1.0], [5.0, 7.5, 2.5]], F)
    eyes = eyes4[np.arange(room.n) % 4]
    with room_context(evplp, room) as c:
        same = c.gather_surface(room.pts, fp, eyes=np.broadcast_to(cam, (room.n, 3)))
        got = c.gather_surface(room.pts, fp, eyes=eyes)
    assert same.tobytes() == base[mode].tobytes(), "eyes = NULL is every eye at camera_pos"
    assert np.array_equal(got["lit"], base[mode]["lit"]) and np.array_equal(got["photons"], base[mode]["photons"])
    assert got[1::4].tobytes() != base[mode][1::4].tobytes()
    for e in range(4):
        sub = np.arange(room.n)[e::4]
        vpl, pm, _ = room.oracle(mode, room.pts[sub], eye=[float(v) for v in eyes4[e]])
        assert_image_close(got["vpl"][sub], vpl, what=f"VPL half, eye {e}")
        assert_image_close(got["pm"][sub], pm, what=f"photon half, eye {e}")


# ---------------------------------------------------------------------------------------------------------------- 5: bytes
def test_a_points_bytes_do_not_depend_on_the_batch_the_form_or_the_buckets(evplp, room, base, monkeypatch):
    import torch
    mode = 5
    fp = evplp.frame_params(**room.params(mode))
    b = base[mode]
    with room_context(evplp, room) as c:
        assert c.gather_surface(room.pts, fp).tobytes() == b.tobytes(), "two runs"
        for i in (0, 777, room.n - 1):
            assert c.gather_surface(room.pts[i:i + 1], fp).tobytes() == b[i:i + 1].tobytes(), i
        for n in (63, 64, 65):
            assert c.gather_surface(room.pts[1000:1000 + n], fp).tobytes() == b[1000:1000 + n].tobytes(), n
        # across the chunk boundary: 16 385 points, copies of the room's in another order
        n = evplp.SURFACE_CHUNK + 1
        src = (np.arange(n) * 7 + 3) % room.n
        got = c.gather_surface(room.pts[src], fp)
        assert got[-1].tobytes() == b[src[-1]].tobytes()
        assert got.tobytes() == b[src].tobytes(), np.nonzero([g.tobytes() != x.tobytes() for g, x in zip(got, b[src])])[0][:8]
        # the device form, two calls enqueued without a wait between them
        d = torch.from_numpy(room.pts.view(F).reshape(-1, 16)).cuda()
        e = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(room.scene.cam_origin, F), (room.n, 3)))).cuda()
        torch.cuda.synchronize()
        x = c.gather_surface(d, fp)
        y = c.gather_surface(d[:65], fp, eyes=e[:65])
        c.synchronize()
        assert isinstance(x, torch.Tensor) and x.is_cuda and tuple(x.shape) == (room.n, 8)
        assert x.cpu().numpy().tobytes() == b.tobytes() and y.cpu().numpy().tobytes() == b[:65].tobytes()
        one = c.gather_surface(room.pts, fp, what=evplp.SURFACE_PHOTONS)
        assert np.array_equal(one["pm"], b["pm"]) and np.array_equal(one["photons"], b["photons"]) and (one["vpl"] == 0).all() and (one["lit"] == 0).all()
    monkeypatch.setenv("EVPLP_SURFACE_GRID_BITS", "4")          # sixteen buckets: every bucket holds many cells
    with room_context(evplp, room) as c:
        assert c.gather_surface(room.pts, fp).tobytes() == b.tobytes(), "EVPLP_SURFACE_GRID_BITS = 4"


# ---------------------------------------------------------------------------------------------------------------- 6: a hostile grid
def floor_box(scene):
    v = np.concatenate([m["verts"] for m in scene.meshes]).astype(F)
    return v.min(0), v.max(0)


def hostile_records(photon_pos):
    """slot 2k the predecessor (above the photon, facing down, Lambertian), slot 2k + 1 photon k"""
    n = len(photon_pos)
    rng = np.random.RandomState(8)
    rec = np.zeros(2 * n, dtype=oa.RECORD_DTYPE)
    up = np.array([0.0, 0.0, 1.0])
    rec["pos"][1::2] = photon_pos; rec["normal"][1::2] = up; rec["flux_dir"][1::2] = up; rec["flux"][1::2] = (0.5 + rng.rand(n, 3)).astype(F)
    rec["rho_d"][1::2] = 0.5; rec["p_select_lambert"][1::2] = 1.0; rec["flags"][1::2] = 2
    rec["pos"][0::2] = photon_pos + np.array([0.3, 0.2, 1.0], F); rec["normal"][0::2] = -up; rec["flux_dir"][0::2] = -up; rec["flux"][0::2] = sd.BIG
    rec["rho_d"][0::2] = (0.2 + 0.6 * rng.rand(n, 3)).astype(F); rec["p_select_lambert"][0::2] = 1.0
    return rec


def floor_points(evplp, X):
    pts = np.zeros(len(X), evplp.SURFACE_POINT_DTYPE)
    pts["pos"] = X; pts["valid"] = 1.0; pts["normal"] = (0.0, 0.0, 1.0); pts["rho_d"] = (0.6, 0.5, 0.4); pts["rho_s"] = (0.2, 0.2, 0.3); pts["phong_exp"] = 20.0
    return pts


@pytest.mark.parametrize("case", ["corners", "huge_radius"])
def test_hostile_grid(evplp, oracle, case):
    scene = sd.floor_scene()
    lo, hi = floor_box(scene)
    rng = np.random.RandomState(9)
    up = F(np.inf)
    if case == "corners":
        r = 0.25
        n_cell = 5000
        edge, bits = evplp.photon_grid_plan(r, lo, hi, 2 * (n_cell + 600))
        # photons on cell corners +- 1 ulp, on the floor
        m = rng.randint(2, 20, (300, 2))
        corner = np.zeros((300, 3), F)
        corner[:, :2] = (lo[:2].astype(np.float64) + m * float(edge)).astype(F)
        step = rng.randint(-1, 2, (300, 2))
        corner[:, :2] = np.where(step > 0, np.nextafter(corner[:, :2], up), np.where(step < 0, np.nextafter(corner[:, :2], -up), corner[:, :2]))
        # 5 000 photons in one cell
        cell0 = lo[:2].astype(np.float64) + np.array([30.0, 12.0]) * float(edge)
        crowd = np.zeros((n_cell, 3), F)
        crowd[:, :2] = (cell0 + rng.uniform(0.02, 0.98, (n_cell, 2)) * float(edge)).astype(F)
        photons = np.concatenate([corner, crowd])
        # points at r (1 +- 2^-23) from the corner photons along x and y, points on the corners, points in and around the crowd
        X = [corner.copy()]
        for sgn, ax in ((1, 0), (-1, 0), (1, 1), (-1, 1)):
            for k in (-1, 0, 1):
                x = corner.astype(np.float64); x[:, ax] += sgn * float(F(r)) * (1.0 + k * 2.0 ** -23); X.append(x.astype(F))
        x = np.zeros((400, 3), F); x[:, :2] = (cell0 + rng.uniform(-1.5, 2.5, (400, 2)) * float(edge)).astype(F); X.append(x)
        X = np.concatenate(X)
    else:
        r = 4.0 * float(np.linalg.norm(hi - lo))        # every photon within the radius of every point near the box, all in a few cells
        photons = np.zeros((700, 3), F); photons[:, :2] = rng.uniform(-11.5, 7.5, (700, 2)).astype(F)
        edge, bits = evplp.photon_grid_plan(r, lo, hi, 1400)
        X = np.zeros((300, 3), F); X[:, :2] = rng.uniform(-11.0, 7.0, (300, 2)).astype(F)
        out = np.zeros((200, 3), F); out[:, :2] = rng.uniform(-2000.0, 2000.0, (200, 2)).astype(F); out[:, 2] = rng.uniform(-500.0, 500.0, 200).astype(F)
        X = np.concatenate([X, out])
    # points outside the box: beside it and far from it
    beside = np.array([[float(lo[0]) - 0.1, 0.0, 0.0], [float(hi[0]) + 0.2, 1.0, 0.0], [0.0, float(lo[1]) - 0.3 * r, 0.0], [0.0, 0.0, -0.5 * r], [1.0e6, 0.0, 0.0]], F)
    X = np.concatenate([X, beside])
    rec = hostile_records(photons)
    pts = floor_points(evplp, X)
    cells = np.stack([evplp.photon_grid_cell(p, lo, edge, bits)[0] for p in photons])
    say(f"hostile grid, {case}: {len(photons)} photons in {len(np.unique(cells, axis=0))} cells (the fullest holds {np.unique(cells, axis=0, return_counts=True)[1].max()}), {len(X)} points, edge {edge:.4g}, {bits} bits")
    want = inside32(photons, X, r).sum(0)
    kw = dict(camera_pos=sd.CAMERA, mis_mode=1, pdf_mc=0.02, clamping_value=0.02, photon_radius=r, num_light_paths=len(photons), num_vpl_light_paths=1, photons_per_path=2)
    with evplp.Context(sd.W, sd.H, len(photons), 1, 2, deterministic=True) as c:
        scene.upload(c)
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        got = c.gather_surface(pts, evplp.frame_params(**kw), what=evplp.SURFACE_PHOTONS)
    assert np.array_equal(got["photons"], want.astype(F)), (case, np.nonzero(got["photons"] != want)[0][:8], got["photons"][:8], want[:8])
    assert want.max() >= (1000 if case == "corners" else 700) and (want == 0).sum() >= 1 and 0 < (want > 0).sum()
    ref, pairs = oa.splat(oa.frame_params(**kw), len(X), 1, planes_of(pts), rec)
    assert pairs == int(want.sum())
    assert_image_close(got["pm"], ref[0, :, :3], what=f"hostile grid, {case}")


# ---------------------------------------------------------------------------------------------------------------- 7: edges and refusals
def test_edges(evplp, room, base):
    mode = 1
    fp = evplp.frame_params(**room.params(mode))
    b = base[mode]
    with room_context(evplp, room) as c:
        assert len(c.gather_surface(np.zeros(0, evplp.SURFACE_POINT_DTYPE), fp)) == 0
        # invalid and stencilled points mixed into a batch; an eye that is not finite
        pts = room.pts[:200].copy()
        live = np.nonzero(room.valid[:200])[0]
        bad = {int(live[3]): ("pos", 0, np.nan), int(live[64]): ("pos", 1, np.inf), int(live[-1]): ("pos", 2, -np.inf)}
        for i, (f, ax, v) in bad.items():
            pts[f][i, ax] = v
        off = [int(live[10]), int(live[65])]
        pts["valid"][off] = 0.0; pts["rho_d"][off] = sd.BIG
        pts["pos"][off[1], 0] = np.nan                       # stencilled AND not finite: the stencil answers
        eyes = np.ascontiguousarray(np.broadcast_to(np.asarray(room.scene.cam_origin, F), (200, 3))).copy()
        bad_eye = int(live[20]); eyes[bad_eye, 1] = np.nan
        got = c.gather_surface(pts, fp, eyes=eyes)
        flat = got.view(F).reshape(-1, 8)
        for i in list(bad) + [bad_eye]:
            assert flat[i].tolist() == [0, 0, 0, -1, 0, 0, 0, -1], (i, flat[i])
        for i in off:
            assert (flat[i] == 0).all(), (i, flat[i])
        ok = np.ones(200, bool); ok[list(bad) + off + [bad_eye]] = False
        assert got[ok].tobytes() == b[:200][ok].tobytes(), "the neighbours are left alone"
        # no usable photon; no usable VPL
        rec = room.records.copy(); rec["flags"] &= ~np.uint32(2)
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        got = c.gather_surface(room.pts, fp)
        assert (got["pm"] == 0).all() and (got["photons"] == 0).all() and np.array_equal(got["vpl"], b["vpl"]) and np.array_equal(got["lit"], b["lit"])
        rec = room.records.copy(); rec["flags"] &= ~np.uint32(1); rec["flux"][(room.records["flags"] & 2) == 0] = sd.BIG
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        got = c.gather_surface(room.pts, fp)
        assert (got["vpl"] == 0).all() and (got["lit"] == 0).all() and np.array_equal(got["photons"], b["photons"])


def test_refusals_leave_the_context_usable_and_write_nothing(evplp, room, base):
    import torch
    L = evplp.lib()
    mode = 1
    pts = room.pts[:8].copy()
    out = np.full(8 * 32, 0x5A, np.uint8)
    xp, op = pts.ctypes.data, out.ctypes.data
    BOTH = evplp.SURFACE_VPL | evplp.SURFACE_PHOTONS
    INV = evplp.ERR_INVALID

    def prm(**kw):
        p = room.params(mode); p.update(kw)
        return C.byref(evplp.frame_params(**p))
    with evplp.Context(W, H, NPATHS, NVPL, P, deterministic=True) as c:               # no evplp_build_accel yet
        assert L.evplp_gather_surface(c._h, prm(), BOTH, xp, None, 8, op) == INV and b"evplp_build_accel" in L.evplp_last_error(c._h)
        assert L.evplp_gather_surface_device(c._h, prm(), BOTH, xp, None, 8, op) == INV
        room.scene.upload(c)
        c.upload(evplp.BUF_RECORDS, room.records.astype(evplp.RECORD_DTYPE))
        for form in (L.evplp_gather_surface, L.evplp_gather_surface_device):
            assert form(c._h, prm(), BOTH, xp, None, -1, op) == INV
            assert form(c._h, prm(), BOTH, None, None, 8, op) == INV and form(c._h, prm(), BOTH, xp, None, 8, None) == INV
            assert form(c._h, None, BOTH, xp, None, 8, op) == INV
            assert form(c._h, prm(), 0, xp, None, 8, op) == INV and form(c._h, prm(), 4, xp, None, 8, op) == INV and form(c._h, prm(), 7, xp, None, 8, op) == INV
            assert form(c._h, prm(mis_mode=6), BOTH, xp, None, 8, op) == INV
            for r in (0.0, -1.0, float("nan"), float("inf")):
                assert form(c._h, prm(photon_radius=r), BOTH, xp, None, 8, op) == INV, r
                assert form(c._h, prm(photon_radius=r), evplp.SURFACE_PHOTONS, xp, None, 8, op) == INV, r
            assert form(c._h, prm(num_vpl_light_paths=0), BOTH, xp, None, 8, op) == INV and form(c._h, prm(photons_per_path=0), BOTH, xp, None, 8, op) == INV
            assert form(c._h, prm(num_light_paths=0), BOTH, xp, None, 8, op) == INV
            assert form(c._h, prm(num_vpl_light_paths=NPATHS + 1), BOTH, xp, None, 8, op) == INV and b"record" in L.evplp_last_error(c._h)
            assert form(c._h, prm(num_light_paths=NPATHS + 1), BOTH, xp, None, 8, op) == INV
            assert form(c._h, prm(photons_per_path=P + 1), BOTH, xp, None, 8, op) == INV
            assert form(c._h, prm(), BOTH, xp, None, 0, op) == evplp.OK and form(c._h, prm(), BOTH, None, None, 0, None) == evplp.OK      # n = 0 touches nothing
        assert (out == 0x5A).all(), "a refused call writes nothing"
        # a radius that is not used is not looked at
        got = c.gather_surface(pts, evplp.frame_params(**dict(room.params(mode), photon_radius=0.0)), what=evplp.SURFACE_VPL)
        assert np.array_equal(got["vpl"], base[mode]["vpl"][:8])
        # the device form's destination must be 16-byte aligned
        d = torch.from_numpy(pts.view(F).reshape(-1, 16)).cuda()
        o = torch.full((8 * 8 + 4,), 7.0, dtype=torch.float32, device="cuda")
        assert L.evplp_gather_surface_device(c._h, prm(), BOTH, C.c_void_p(d.data_ptr()), None, 8, C.c_void_p(o.data_ptr() + 4)) == INV
        assert b"aligned" in L.evplp_last_error(c._h)
        c.synchronize()
        assert (o.cpu().numpy() == 7.0).all()
        assert c.gather_surface(pts, evplp.frame_params(**room.params(mode))).tobytes() == base[mode][:8].tobytes(), "the context is usable afterwards"
        # dirty vertices: refused until the refit
        c.transform_mesh(6 + 5, [1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, 1, 0])
        assert L.evplp_gather_surface(c._h, prm(), BOTH, xp, None, 8, op) == INV and b"evplp_refit_accel" in L.evplp_last_error(c._h)
        assert (out == 0x5A).all()


# ---------------------------------------------------------------------------------------------------------------- 8: a moved occluder
def test_a_moved_occluder_is_followed_after_the_refit(evplp, room, base):
    mesh = 6 + 5                                    # the top face of the first box: doubled and lifted under the light
    centre = room.scene.meshes[mesh]["verts"].mean(0)
    s = 2.0
    t = np.array([4.2, 3.9, 3.6]) - s * centre
    fp = evplp.frame_params(**room.params(0))
    with room_context(evplp, room) as c:
        c.transform_mesh(mesh, [s, 0, 0, t[0], 0, s, 0, t[1], 0, 0, s, t[2]])
        with pytest.raises(evplp.EvplpError) as e:
            c.gather_surface(room.pts, fp)
        assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value)
        c.refit_accel()
        got = c.gather_surface(room.pts, fp, what=evplp.SURFACE_VPL)
        now = scenes.moved(room.scene)              # (a copy: scale 1, no offset) with the occluder where the context has it
        now.meshes[mesh]["verts"] = c.mesh_vertices(mesh, 0)
        assert not np.array_equal(now.meshes[mesh]["verts"], room.scene.meshes[mesh]["verts"])
        now.triangle_soup()
    lit, _ = room.brute_lit(oa.Scene(now))
    changed = int((lit != room.lit).sum())
    say(f"moved occluder: {changed} points changed their lit count")
    assert changed > 50
    assert np.array_equal(got["lit"], np.where(room.valid, lit, 0).astype(F)), np.nonzero(got["lit"] != lit)[0][:8]


# ---------------------------------------------------------------------------------------------------------------- 9: the frame's own passes
def test_agreement_with_the_frames_gather_and_splat(evplp, room):
    """The context's own G-buffer as the point list: gather_lvc with a window of all paths and splat_photons(IDEAL) each lie within one bar
    of the oracle, as this call does: twice the bars between them.  The pass that counts lit pairs is gather_vpl (rays, shaded); gather_lvc
    counts its shadow rays alone, which must be this call's pairs that pass the cosine test."""
    n, p, mode = 160, 4, 1
    kw = dict(camera_pos=room.scene.cam_origin, mis_mode=mode, pdf_mc=1.0 / (np.pi * room.radius ** 2), clamping_value=0.05, photon_radius=room.radius,
              num_light_paths=n, num_vpl_light_paths=n, photons_per_path=p, rng_seed=3)
    fp = evplp.frame_params(**kw)
    with evplp.Context(W, H, n, n, p, deterministic=True) as c:
        room.scene.upload(c)
        c.primary((0.0, 0.0), clear_light=True)
        c.trace_light_paths(3)
        c.clear_accumulators()
        c.gather_lvc(fp)
        lvc = c.download(evplp.BUF_VPL_ACCUM)[:H].reshape(-1, 4)[:, :3]
        c.clear_accumulators()
        c.gather_vpl(fp)
        shaded = c.pass_stats(evplp.PASS_GATHER_VPL)["shaded"]
        c.splat_photons(fp, clear=True)
        pm = c.download(evplp.BUF_PHOTON_ACCUM)[:H].reshape(-1, 4)[:, :3]
        pairs = c.pass_stats(evplp.PASS_SPLAT)["pairs"]
        gbuf = [c.download(b)[:H] for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG)]
        pts = points_of(evplp, gbuf)
        got = c.gather_surface(pts, fp)
    valid = pts["valid"] != 0
    assert valid.sum() > 0.9 * len(pts)
    assert int(got["lit"].sum()) == shaded and shaded > 10000, (got["lit"].sum(), shaded)
    say(f"frame: VPL half against gather_lvc rel L2 {rel_l2(got['vpl'], lvc):.2e}, photon half against splat_photons {rel_l2(got['pm'][valid], pm[valid]):.2e}; {shaded} lit pairs")
    assert_image_close(got["vpl"], lvc, rel=2 * REL_L2, pix=2 * PIX_REL, what="VPL half against gather_lvc")
    # (the splat has no stencil: a pixel that shows nothing still collects photons around its cleared position; a point with valid = 0 answers zeros)
    assert_image_close(got["pm"][valid], pm[valid], rel=2 * REL_L2, pix=2 * PIX_REL, what="photon half against splat_photons")
    assert int(got["photons"].sum()) == pairs if valid.all() else int(got["photons"].sum()) <= pairs
