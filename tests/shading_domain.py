"""Inputs that visit every arm of the pair shading, and its float64 restatement (numpy only; the oracle serves once, for the floor's
primary G-buffer, in Domain).

The shading of one (pixel, VPL) pair -- vplSplat after its visibility test, rt/lighttracing.cu:275-346 with the helpers of
rt/rtmaterial.cuh -- and of one (pixel, photon) fragment -- shaders/photonsplatinstanced.frag:146-240 -- is restated here in float64
on the float32 inputs, the way vpl_shade / evo_photon_frag of oracle/evplp_oracle.c restate them in float32.  Quirks of the
reference that are kept (and where they are):
  * PhongEvalF has no reflectance test (rtmaterial.cuh:112-118); PhongPdfA tests phongReflectance.x alone, against 1e-6 (:92);
    the fragment shader's PhongPdfW tests .x against 1e-5 (frag:83) and its PhongEval tests nothing but the cosine (frag:56).
  * PhongPdfA normalises the reflected direction (rtmaterial.cuh:90), PhongEvalF and the GLSL helpers do not (:114, frag:54,81).
  * the lobe cut is `cos <= 1e-6` in CUDA (rtmaterial.cuh:92,116) and `<= 1e-5` in GLSL (frag:56,83).
  * LambertPdfA carries 1/pi (rtmaterial.cuh:53); the CUDA LambertPdfW does not (:40-44) but vplSplat never calls it; the GLSL
    LambertPdfW does (frag:65-69).
  * misMode 5 of the fragment shader divides by geometryTerm * brdf2 per channel (frag:232); a zero channel of brdf2 contributes 0
    here as in the oracle and the kernels (the reference's NaN).

Every evaluation returns, next to the value, how well conditioned it is:
  kappa   1 + sum e / d over the lobe powers taken + sum 1 / cos over the cosines that are differences (-n2 . v12, n1 . w12, ...)
          + x / (x - clamp) where a splat clamp subtracts (modes 4 and 5).  An error of a few 2^-24 in a cosine d moves d^e by e / d
          times that, a cosine that is a difference of products has 1 / cos times the rounding of its terms.
  lam     sum e |log2 d| over the powers the kernels take as exp2(e log2 d) on the hardware transcendentals (kernels_gather.hip:41-44
          bounds that error by 0.7 2^-22 lam)
  decided False where a discrete comparison of the formulas lies within its margin: a clamped cosine within 4e-6 of 0, a lobe cosine
          within 4e-6 of 0 or of the cut, |pdf_mc - pdf| < 1e-3 pdf_mc under the max heuristic, a clamp subtraction within 1e-4
          (relative) of 0, the splat's radius within 1e-4 (relative).  Such pairs are compared with nothing.
"""
import math
from types import SimpleNamespace

import numpy as np

W, H = 44, 28                 # 6 x 4 tiles of 8 x 8 pixels; the last column is 4 pixels wide, the last row 4 pixels high
NPATHS, P = 32, 2             # 64 record slots; 1 / NPATHS is exact, so the division of lighttracing.cu:378 adds no rounding
E_SET = (0.0, 0.5, 1.0, 20.0, 200.0, 1000.0)
CAMERA = (0.0, 0.0, 10.0)     # straight down on the floor z = 0; x to the right, y up the image
FOVY = math.radians(60.0)
PDF_MC = 0.02
CLAMP = 0.02
RADIUS = 1.0                  # 2.4 pixels: a footprint is 4 - 5 pixels across
BIG = 1.0e30                  # what an unusable slot or a stencilled-out pixel carries: finite, and ruinous if it were read

COS_MARGIN = 4.0e-6
CUT_CUDA = float(np.float32(0.000001))
CUT_GLSL = float(np.float32(0.00001))
INV_PI = 1.0 / math.pi

# tile classes [tile row][tile column]; tile row 3 and tile column 5 are ragged
TILES = [
    ["lambert", "glossy", "one_lane0", "one_lane63", "one_mid", "glossy"],
    ["rsx_zero", "rsx_tiny", "pure_spec", "stencil", "lambert", "one_lane0"],
    ["glossy", "pure_spec", "one_mid", "lambert", "rsx_zero", "rsx_tiny"],
    ["lambert", "one_lane0", "one_mid", "rsx_zero", "pure_spec", "stencil"],
]
TILE_CLASSES = ("lambert", "glossy", "one_lane0", "one_lane63", "one_mid", "rsx_zero", "rsx_tiny", "pure_spec", "stencil")
RAGGED_CLASSES = tuple(c for c in TILE_CLASSES if c != "one_lane63")          # (lane 63 of a ragged tile is outside the frame)
PIXEL_CLASSES = ("lambert_e_left", "glossy", "rsx_zero", "rsx_tiny", "pure_spec", "stencil_off") + tuple(f"e_{e:g}" for e in E_SET)


def floor_scene():
    """one quad z = 0 under the whole frame and a small light quad far above every VPL: nothing occludes anything"""
    import scenes
    s = scenes.SceneData()
    s.aspect = W / H
    floor = s.add_material((0.5, 0.5, 0.5))
    s.add_quad([-12.0, -8.0, 0.0], [24.0, 0.0, 0.0], [0.0, 16.0, 0.0], floor)
    lm = s.add_material((0, 0, 0))
    s.light_mesh = s.add_quad([-0.5, -0.5, 90.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], lm)
    s.light_intensity = [1.0, 1.0, 1.0, 0.0]
    s.cam_origin = list(CAMERA); s.cam_lookat = [0.0, 0.0, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.fovy = FOVY
    s.triangle_soup()
    return s


def _mirror(v, n):
    """reflect(-v, n) of optixu_math: v mirrored about n"""
    v = np.asarray(v, np.float64); n = np.asarray(n, np.float64)
    return 2.0 * n * np.dot(n, v) - v


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt(np.dot(v, v))


# ------------------------------------------------------------------------------------------------------------------ receiver
def make_receiver(pos_plane, nrm_plane):
    """the G-buffer: positions and normals of the floor as the primary pass wrote them, reflectances by tile class.
    Returns ([pos, nrm, dif, phg] float32 [H, W, 4], pixel class names [H, W] (object array of tuples))"""
    pos = np.array(pos_plane, np.float32, copy=True); nrm = np.array(nrm_plane, np.float32, copy=True)
    assert pos.shape == (H, W, 4) and np.all(pos[..., 3] == 1.0) and np.all(pos[..., 2] == 0.0), "the floor fills the frame"
    assert np.all(nrm[..., :3] == np.array([0, 0, 1], np.float32)), "the floor's normal is exactly (0, 0, 1)"
    rng = np.random.RandomState(20261)
    dif = np.zeros((H, W, 4), np.float32); phg = np.zeros((H, W, 4), np.float32)
    rd = (0.2 + 0.6 * rng.rand(H, W, 3)).astype(np.float32)
    rs = (0.1 + 0.4 * rng.rand(H, W, 3)).astype(np.float32)
    e = np.asarray(E_SET, np.float32)[rng.randint(0, len(E_SET), size=(H, W))]
    stencil_off = rng.rand(H, W) < 0.3
    names = np.empty((H, W), dtype=object)
    for y in range(H):
        for x in range(W):
            cls = TILES[y >> 3][x >> 3]; lane = (y & 7) * 8 + (x & 7)
            glossy_px = dict(one_lane0=lane == 0, one_lane63=lane == 63, one_mid=lane == 27).get(cls, cls != "lambert")
            dif[y, x, :3] = rd[y, x]
            tags = []
            if not glossy_px:
                phg[y, x] = (0.0, 0.0, 0.0, 37.0)                      # a Lambert pixel with an exponent left in the plane
                tags.append("lambert_e_left")
            else:
                ee = dict(one_lane0=20.0, one_lane63=1000.0, one_mid=0.5).get(cls, e[y, x])
                phg[y, x, :3] = rs[y, x]; phg[y, x, 3] = ee
                tags += ["glossy", f"e_{float(ee):g}"]
                if cls == "rsx_zero":
                    phg[y, x, 0] = 0.0; tags.append("rsx_zero")
                if cls == "rsx_tiny":
                    phg[y, x, 0] = 5.0e-7; tags.append("rsx_tiny")
                if cls == "pure_spec":
                    dif[y, x, :3] = 0.0; tags.append("pure_spec")
                if cls == "stencil" and stencil_off[y, x]:
                    pos[y, x, 3] = 0.0; dif[y, x, :3] = BIG; phg[y, x, :3] = BIG; tags.append("stencil_off")
            names[y, x] = tuple(tags)
    return [pos, nrm, dif, phg], names


def pixels_of(gbuf):
    pos, nrm, dif, phg = gbuf
    return SimpleNamespace(pos=pos[..., :3].astype(np.float64), stencil=pos[..., 3] != 0.0, nrm=nrm[..., :3].astype(np.float64),
                           rd=dif[..., :3].astype(np.float64), rs=phg[..., :3].astype(np.float64), e=phg[..., 3].astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ records
def _record_dtype():
    import oracle_api as oa
    return oa.RECORD_DTYPE


def _fill(rec, k, pos, normal, fdir, flux, rd, rs, e, psel, flags):
    rec["pos"][k] = pos; rec["normal"][k] = _unit(normal); rec["flux_dir"][k] = _unit(fdir); rec["flux"][k] = flux
    rec["rho_d"][k] = rd; rec["rho_s"][k] = rs; rec["phong_exp"][k] = e; rec["p_select_lambert"][k] = psel; rec["flags"][k] = flags


def make_vpls():
    """(records [NPATHS * P] with every class usable, class name per used slot).  Unused slots: flags 0, flux 1e30."""
    rng = np.random.RandomState(20262)
    down = np.array([0.0, 0.0, -1.0])
    out = []

    def add(name, pos, e=0.0, psel=1.0, rs=None, rd=None, normal=down, aim=None, fdir=None, flux=None):
        pos = np.asarray(pos, np.float64); normal = _unit(normal)
        if fdir is None:                    # the lobe's axis reflect(-fdir, n) points at `aim` on the floor (default: a pixel near below)
            aim = np.array([0.6 * pos[0] + 0.5, 0.6 * pos[1] - 0.4, 0.0]) if aim is None else np.asarray(aim, np.float64)
            fdir = _mirror(_unit(aim - pos), normal)
        rd = 0.2 + 0.6 * rng.rand(3) if rd is None else rd
        rs = (0.0, 0.0, 0.0) if rs is None else rs
        flux = 0.5 + 1.5 * rng.rand(3) if flux is None else flux
        out.append((name, pos, normal, fdir, flux, rd, rs, e, psel))

    def spot():
        return np.array([-8.0 + 16.0 * rng.rand(), -5.0 + 10.0 * rng.rand(), 0.0])

    def gl():
        return 0.1 + 0.4 * rng.rand(3)

    for h in (1.0e-3, 0.05, 0.5, 3.0, 50.0):
        add(f"lambert_h{h:g}", spot() + [0, 0, h])
    add("on_light", spot() + [0, 0, 3.0], e=0.0, psel=1.0, rd=(1.0, 1.0, 1.0))
    for e in E_SET:
        add(f"glossy_e{e:g}_p0.3", spot() + [0, 0, (0.5, 3.0)[int(e) % 2]], e=e, psel=0.3, rs=gl())
    for e in (0.0, 20.0, 200.0, 1000.0):
        for psel in (0.0, 1.0):
            add(f"glossy_e{e:g}_p{psel:g}", spot() + [0, 0, 1.5], e=e, psel=psel, rs=gl())
    for h in (1.0e-3, 0.05, 50.0):
        add(f"glossy_h{h:g}", spot() + [0, 0, h], e=20.0, psel=0.3, rs=gl())
    add("rsx_zero", spot() + [0, 0, 1.0], e=20.0, psel=0.3, rs=(0.0, 0.3, 0.2))
    add("rsx_tiny", spot() + [0, 0, 1.0], e=20.0, psel=0.3, rs=(5.0e-7, 0.3, 0.2))
    add("rho_d_zero", spot() + [0, 0, 1.0], e=20.0, psel=0.0, rs=gl(), rd=(0.0, 0.0, 0.0))
    add("lobe_at_frame", [3.0, -2.0, 2.0], e=200.0, psel=0.3, rs=gl(), aim=[-1.0, 1.0, 0.0])
    add("lobe_away", [9.5, 0.0, 0.5], e=20.0, psel=0.3, rs=gl(), fdir=_mirror(_unit([1.0, 0.0, -0.02]), down))
    add("lobe_e0_edge", [0.3, 0.2, 1.0], e=0.0, psel=0.3, rs=gl(), fdir=_mirror(_unit([1.0, 0.13, -0.3]), down))
    for deg in (30.0, 60.0, 85.0, 89.9):
        t = math.radians(deg)
        add(f"tilt_{deg:g}", [-2.0 + 0.01 * deg, 0.7, 1.0], normal=[math.sin(t), 0.0, -math.cos(t)])
    t = math.radians(75.0)
    add("tilt_glossy", [1.1, -1.3, 0.8], e=20.0, psel=0.3, rs=gl(), normal=[-math.sin(t), 0.0, -math.cos(t)], aim=[4.0, -1.0, 0.0])
    add("facing_away", [1.0, 1.0, 2.0], normal=[0.0, 0.0, 1.0], fdir=[0.0, 0.0, 1.0])
    add("below_floor", [1.0, -1.0, -0.5], e=20.0, psel=0.3, rs=gl(), fdir=[0.3, 0.0, -1.0])
    add("zero_flux", spot() + [0, 0, 1.0], e=20.0, psel=0.3, rs=gl(), flux=(0.0, 0.0, 0.0))

    rec = np.zeros(NPATHS * P, dtype=_record_dtype())
    rec["flux"] = BIG
    assert len(out) <= len(rec)
    for k, (name, *fields) in enumerate(out):
        _fill(rec, k, *fields, flags=1)
    return rec, [o[0] for o in out]


DARK_VPLS = ("facing_away", "below_floor", "zero_flux")       # contribute exactly 0 everywhere


def only_slot(records, k, flag):
    """the records with slot k alone usable; every other slot: flags 0, flux 1e30 (the rest of it stays: a photon's predecessor is read)"""
    r = records.copy()
    r["flags"] = 0; r["flags"][k] = flag
    keep = r["flux"][k].copy(); r["flux"] = BIG; r["flux"][k] = keep
    return r


def make_photons(pos_plane):
    """(records: slot 2k the predecessor, slot 2k + 1 photon k (flag 2); class names; photon slots)."""
    rng = np.random.RandomState(20263)
    px = float(pos_plane[0, 1, 0] - pos_plane[0, 0, 0])
    up = np.array([0.0, 0.0, 1.0]); down = -up
    cam = np.asarray(CAMERA, np.float64)
    offs = [(0, 0), (4, 3), (7, 4), (3, 7), (1, 2), (6, 6)]
    out = []

    def gl():
        return 0.1 + 0.4 * rng.rand(3)

    def photon_pos(k):
        tx, ty = k % 6, k // 6
        ox, oy = offs[(k + ty) % len(offs)]
        x, y = min(tx * 8 + ox, W - 2), min(ty * 8 + oy, H - 2)
        return np.array([pos_plane[y, x, 0] + 0.37 * px, pos_plane[y, x, 1] + 0.21 * px, 0.0], np.float64)

    def add(name, rel, e=0.0, psel=1.0, rs=None, rd=None, normal=down, fdir="at_photon", flux=None):
        k = len(out)
        ppos = photon_pos(k)
        rel = np.asarray(rel, np.float64); normal = _unit(normal)
        if isinstance(fdir, str):           # the predecessor's lobe axis points at the photon
            fdir = _mirror(_unit(-rel), normal)
        rd = 0.2 + 0.6 * rng.rand(3) if rd is None else rd
        rs = (0.0, 0.0, 0.0) if rs is None else rs
        flux = 0.5 + 1.5 * rng.rand(3) if flux is None else flux
        out.append((name, ppos, ppos + rel, normal, fdir, flux, rd, rs, e, psel))

    for h in (0.5, 0.05, 3.0, 10.0):
        add(f"lambert_h{h:g}", [0.3 * h, 0.2 * h, h])
    add("on_light", [0.4, -0.3, 6.0], rd=(1.0, 1.0, 1.0))
    for i, e in enumerate(E_SET):
        h = (0.5, 1.0, 3.0)[i % 3]
        add(f"glossy_e{e:g}_p0.3", [-0.35 * h, 0.15 * h, h], e=e, psel=0.3, rs=gl())
    add("glossy_p0", [0.2, 0.5, 1.0], e=20.0, psel=0.0, rs=gl())
    add("glossy_p1", [0.2, -0.5, 7.0], e=20.0, psel=1.0, rs=gl())
    # w12 mirrored about the floor's normal points at the camera: the receivers' own lobes peak inside the footprint
    pp = photon_pos(len(out)); m = _unit(cam - pp)
    add("mirror_of_camera", 2.0 * np.array([-m[0], -m[1], m[2]]), e=200.0, psel=0.0, rs=gl())
    add("rsx_zero", [0.3, 0.1, 1.0], e=20.0, psel=0.3, rs=(0.0, 0.3, 0.2))
    add("rsx_tiny", [-0.3, 0.1, 1.0], e=20.0, psel=0.3, rs=(5.0e-7, 0.3, 0.2))
    add("rho_d_zero", [0.1, 0.3, 0.5], e=20.0, psel=0.0, rs=gl(), rd=(0.0, 0.0, 0.0))
    add("lobe_away", [0.2, 0.2, 1.0], e=20.0, psel=0.3, rs=gl(), fdir=_mirror(_unit([1.0, 0.0, -0.05]), down))
    t = math.radians(60.0)
    add("tilt_60", [0.5, 0.1, 1.0], normal=[math.sin(t), 0.0, -math.cos(t)])
    t = math.radians(85.0)
    add("tilt_85", [0.9, 0.1, 0.5], e=20.0, psel=0.3, rs=gl(), normal=[math.sin(t), 0.0, -math.cos(t)])
    add("mix_w_zero", [0.2, 0.1, 1.0], e=20.0, psel=0.0, rs=(0.0, 0.3, 0.2))
    add("cc_zero", [0.2, 0.1, 1.0], e=20.0, psel=0.3, rs=gl(), normal=up, fdir=_unit([0.2, 0.1, -1.0]))
    add("brdf2_zero_channel", [0.1, -0.2, 0.4], e=20.0, psel=0.3, rs=(0.2, 0.0, 0.1), rd=(0.5, 0.0, 0.3))
    add("zero_flux", [0.1, 0.2, 1.0], flux=(0.0, 0.0, 0.0))

    rec = np.zeros(NPATHS * P, dtype=_record_dtype())
    rec["flux"] = BIG
    assert len(out) == 24 and 2 * len(out) <= len(rec)
    for k, (name, ppos, prev_pos, normal, fdir, flux, rd, rs, e, psel) in enumerate(out):
        _fill(rec, 2 * k, prev_pos, normal, fdir, BIG, rd, rs, e, psel, flags=0)
        _fill(rec, 2 * k + 1, ppos, up, up, flux, (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), 0.0, 1.0, flags=2)
    return rec, [o[0] for o in out], [2 * k + 1 for k in range(len(out))]


VPL_CLASSES = ("lambert_h", "on_light", "glossy_e", "glossy_h", "rsx_zero", "rsx_tiny", "rho_d_zero", "lobe_at_frame", "lobe_away", "lobe_e0_edge",
               "tilt_", "tilt_glossy", "facing_away", "below_floor", "zero_flux") + tuple(f"glossy_e{e:g}_" for e in E_SET) + ("_p0", "_p0.3", "_p1")
PHOTON_CLASSES = ("lambert_h", "on_light", "glossy_e", "glossy_p0", "glossy_p1", "mirror_of_camera", "rsx_zero", "rsx_tiny", "rho_d_zero", "lobe_away",
                  "tilt_60", "tilt_85", "mix_w_zero", "cc_zero", "brdf2_zero_channel", "zero_flux")


def coverage(pixel_names, vpl_names, photon_names):
    """how many pixels / tiles / records every class of the inputs has -- the tests assert none is empty"""
    c = {}
    for cls in PIXEL_CLASSES:
        c["pixel:" + cls] = sum(cls in t for t in pixel_names.ravel())
    for cls in TILE_CLASSES:
        c["tile:" + cls] = sum(TILES[ty][tx] == cls for ty in range(3) for tx in range(5))
    for cls in RAGGED_CLASSES:
        c["ragged_tile:" + cls] = sum(TILES[ty][tx] == cls for ty in range(4) for tx in range(6) if ty == 3 or tx == 5)
    for cls in VPL_CLASSES:
        c["vpl:" + cls] = sum(cls in n for n in vpl_names)
    for cls in PHOTON_CLASSES:
        c["photon:" + cls] = sum(cls in n for n in photon_names)
    return c


# ------------------------------------------------------------------------------------------------------------------ float64
def params(mode, num_light_paths=NPATHS, num_vpl_light_paths=NPATHS, photons_per_path=P, do_accumulate=0):
    """keyword arguments of both frame_params constructors (oracle_api, evplp_amd)"""
    return dict(camera_pos=CAMERA, mis_mode=mode, pdf_mc=PDF_MC, clamping_value=CLAMP, photon_radius=RADIUS, num_light_paths=num_light_paths,
                num_vpl_light_paths=num_vpl_light_paths, photons_per_path=photons_per_path, do_accumulate=do_accumulate)


def _f(x):
    return float(np.float32(x))


def _dot(a, b):
    return (a * b).sum(-1)


def _rec64(r):
    g = lambda k: np.asarray(r[k], np.float64)
    return SimpleNamespace(pos=g("pos"), n=g("normal"), flux=g("flux"), fdir=g("flux_dir"), rd=g("rho_d"), rs=g("rho_s"), e=float(r["phong_exp"]),
                           psel=float(r["p_select_lambert"]))


def _near_cut(d, cut):
    return (np.abs(d) < COS_MARGIN) | (np.abs(d - cut) < COS_MARGIN)


def _pow(d, e):
    return np.power(np.maximum(d, 1e-300), e)


def vpl_pair_f64(mode, fp, pixel, record):
    """vplSplat (rt/lighttracing.cu:275-346) of every pixel of `pixel` (pixels_of) with one record, visibility = 1, in float64.
    fp: params(mode).  Returns value [..., 3] (NOT divided by numVplLightPaths), kappa [...], lam [...], decided [...], lit [...]
    (lit: the pair passes the stencil of :354 and the cosine test of :288 -- it casts a shadow ray)."""
    v = _rec64(record)
    cam = np.asarray([_f(c) for c in fp["camera_pos"]], np.float64)
    pdf_mc, clamp = _f(fp["pdf_mc"]), _f(fp["clamping_value"])
    p1, n1 = pixel.pos, pixel.nrm
    v12 = v.pos - p1                                                            # :282
    c1u, c2u = _dot(n1, v12), -_dot(v12, v.n)
    c1c2 = np.maximum(c1u, 0.0) * np.maximum(c2u, 0.0)                          # :284-286
    lit = pixel.stencil & (c1c2 > 0.0)                                          # :288, :354
    dist2 = _dot(v12, v12); dist = np.sqrt(dist2)
    wi12 = v12 / dist[..., None]                                                # :299
    cos1, cos2 = c1u / dist, c2u / dist
    decided = ~(np.abs(cos1) < COS_MARGIN) & ~(np.abs(cos2) < COS_MARGIN)
    d10 = cam - p1; wi10 = d10 / np.sqrt(_dot(d10, d10))[..., None]             # :363
    kappa = 1.0 + 1.0 / np.maximum(cos1, 1e-300) + 1.0 / np.maximum(cos2, 1e-300)
    lam = np.zeros_like(dist)
    # PhongEvalF(-wi12, fluxDir, n2, e2), rtmaterial.cuh:112-118
    lobe2 = bool(np.any(v.rs != 0.0))
    d2 = _dot(-wi12, 2.0 * v.n * np.dot(v.n, v.fdir) - v.fdir)
    on2 = d2 > CUT_CUDA
    ph2 = np.where(on2, (v.e + 2.0) * _pow(d2, v.e) * INV_PI * 0.5, 0.0)
    if lobe2:
        decided &= ~_near_cut(d2, CUT_CUDA)
        kappa = kappa + np.where(on2, v.e / np.maximum(d2, CUT_CUDA), 0.0)
        lam = lam + np.where(on2, v.e * np.abs(np.log2(np.maximum(d2, CUT_CUDA))), 0.0)
    # PhongEvalF(wi10, wi12, n1, e1)
    lobe1 = np.any(pixel.rs != 0.0, axis=-1)
    r1 = 2.0 * n1 * _dot(n1, wi12)[..., None] - wi12
    d1 = _dot(wi10, r1)
    on1 = d1 > CUT_CUDA
    ph1 = np.where(on1, (pixel.e + 2.0) * _pow(d1, pixel.e) * INV_PI * 0.5, 0.0)
    decided &= ~(lobe1 & _near_cut(d1, CUT_CUDA))
    kappa = kappa + np.where(lobe1 & on1, pixel.e / np.maximum(d1, CUT_CUDA), 0.0)
    lam = lam + np.where(lobe1 & on1, pixel.e * np.abs(np.log2(np.maximum(d1, CUT_CUDA))), 0.0)
    brdf2 = v.rd * INV_PI + v.rs * ph2[..., None]                               # :302-303
    brdf1 = pixel.rd * INV_PI + pixel.rs * ph1[..., None]                       # :305-306
    g21 = c1c2 / (dist2 * dist2)                                                # :308
    if mode == 0:
        val = v.flux * brdf1 * brdf2 * g21[..., None]
    elif mode <= 3:
        pdf_de = g21 * INV_PI * v.psel                                          # LambertPdfA(n2, n1, -v12), rtmaterial.cuh:46-54
        if not v.rs[0] <= CUT_CUDA:                                             # PhongPdfA, :87-102: .x alone, reflected direction normalised
            r = 2.0 * v.n * np.dot(v.n, v.fdir) - v.fdir; r = r / math.sqrt(np.dot(r, r))
            c = _dot(-wi12, r)
            onp = c > CUT_CUDA
            pdfw = np.where(onp, (v.e + 1.0) * 0.5 * INV_PI * _pow(c, v.e), 0.0)
            pdf_de = pdf_de + pdfw * np.maximum(cos1, 0.0) / dist2 * (1.0 - v.psel)
            if v.psel != 1.0:
                decided &= ~_near_cut(c, CUT_CUDA)
                kappa = kappa + np.where(onp, v.e / np.maximum(c, CUT_CUDA), 0.0)
        if mode == 1:
            w = pdf_mc / (pdf_mc + pdf_de)
        elif mode == 2:
            w = np.where(pdf_mc > pdf_de, 1.0, 0.0)
            decided &= ~(np.abs(pdf_mc - pdf_de) < 1.0e-3 * pdf_mc)
        else:
            w = pdf_mc * pdf_mc / (pdf_mc * pdf_mc + pdf_de * pdf_de)
        val = v.flux * w[..., None] * brdf1 * brdf2 * g21[..., None]
    elif mode == 4:
        val = v.flux * np.minimum(g21, clamp)[..., None] * brdf1 * brdf2        # :340
    else:
        val = v.flux * np.minimum(brdf1 * g21[..., None] * brdf2, clamp)        # :344
    val = np.where(lit[..., None], val, 0.0)
    return val, np.where(lit, kappa, 1.0), np.where(lit, lam, 0.0), decided, lit


def photon_frag_f64(mode, fp, pixel, photon, prev):
    """main() of shaders/photonsplatinstanced.frag:146-240 for every pixel of `pixel` with one photon and its predecessor on the light
    path, in float64.  Returns value [..., 3], kappa [..., 3], lam [...], decided [...], inside [...] (the radius test of :152-154)
    and radius_decided [...]."""
    ph, pv = _rec64(photon), _rec64(prev)
    cam = np.asarray([_f(c) for c in fp["camera_pos"]], np.float64)
    pdf_mc, clamp, r = _f(fp["pdf_mc"]), _f(fp["clamping_value"]), _f(fp["photon_radius"])
    X, sn = pixel.pos, pixel.nrm
    dv = ph.pos - X
    dist = np.sqrt(_dot(dv, dv))
    inside = ~(_dot(dv, dv) > r * r)                                            # :153-154
    radius_decided = ~(np.abs(dist - r) < 1.0e-4 * r)
    v12 = pv.pos - ph.pos                                                       # :170
    d2 = float(np.dot(v12, v12)); w12 = v12 / math.sqrt(d2)
    d10 = cam - X; w10 = d10 / np.sqrt(_dot(d10, d10))[..., None]               # :177
    decided = np.ones(X.shape[:-1], bool)
    kappa = np.ones(X.shape[:-1])
    lam = np.zeros(X.shape[:-1])
    # brdf1 = LambertEval(w10, w12, sn, rd) + PhongEval(w10, w12, sn, rs, e), :181
    ca, cb = _dot(w10, sn), _dot(sn, w12)
    lam1 = np.where(((ca <= 0.0) | (cb <= 0.0))[..., None], 0.0, pixel.rd * INV_PI)
    decided &= ~(np.abs(ca) < COS_MARGIN) & ~(np.abs(cb) < COS_MARGIN)
    lobe1 = np.any(pixel.rs != 0.0, axis=-1)
    d1 = _dot(w10, 2.0 * sn * cb[..., None] - w12)
    on1 = d1 > CUT_GLSL
    pe1 = np.where(on1[..., None], pixel.rs * ((pixel.e + 2.0) * _pow(d1, pixel.e) * INV_PI * 0.5)[..., None], 0.0)
    decided &= ~(lobe1 & _near_cut(d1, CUT_GLSL))
    kappa = kappa + np.where(lobe1 & on1, pixel.e / np.maximum(d1, CUT_GLSL), 0.0)
    lam = lam + np.where(lobe1 & on1, pixel.e * np.abs(np.log2(np.maximum(d1, CUT_GLSL))), 0.0)
    brdf1 = lam1 + pe1
    # mixPdfW, :184-187 (GLSL LambertPdfW carries 1/pi; PhongPdfW: .x alone against 1e-5, reflected direction not normalised)
    cl = float(np.dot(pv.n, -w12))
    mix_w = max(cl, 0.0) * INV_PI * pv.psel
    rp = 2.0 * pv.n * np.dot(pv.n, pv.fdir) - pv.fdir
    dp = float(np.dot(-w12, rp))
    record_decided = True
    k_pdf, lam_pdf = 0.0, 0.0
    if pv.psel != 0.0:
        record_decided &= not abs(cl) < COS_MARGIN
        if cl > 0.0:
            k_pdf += 1.0 / cl
    if pv.psel != 1.0 and not pv.rs[0] <= CUT_GLSL:
        record_decided &= not bool(_near_cut(np.float64(dp), CUT_GLSL))
        if dp > CUT_GLSL:
            mix_w += (pv.e + 1.0) * 0.5 * INV_PI * dp ** pv.e * (1.0 - pv.psel)
            k_pdf += pv.e / dp; lam_pdf += pv.e * abs(math.log2(dp))
    cn = float(np.dot(ph.n, w12))
    mix_a = mix_w * max(cn, 0.0) / d2                                           # :189
    alive = mix_w > 0.0                                                         # :191
    k = INV_PI / (r * r); inv_n = 1.0 / float(fp["num_light_paths"])
    base = brdf1 * k * ph.flux * inv_n
    if mode == 0:
        val = base
    elif mode <= 3:
        record_decided &= not abs(cn) < COS_MARGIN
        kappa = kappa + k_pdf + (1.0 / cn if cn > 0.0 else 0.0); lam = lam + lam_pdf
        if mode == 1:
            w = mix_a / (mix_a + pdf_mc)
        elif mode == 2:
            w = 1.0 if mix_a > pdf_mc else 0.0
            record_decided &= not abs(mix_a - pdf_mc) < 1.0e-3 * pdf_mc
        else:
            w = mix_a * mix_a / (mix_a * mix_a + pdf_mc * pdf_mc)
        val = base * w
    else:
        cpn = float(np.dot(pv.n, w12))
        cc = np.maximum(cb, 0.0) * max(-cpn, 0.0)                               # :218, :228
        record_decided &= not abs(cpn) < COS_MARGIN
        keep = cc > 0.0
        g = np.where(keep, cc, 1.0) / d2
        kappa = kappa + np.where(keep, 1.0 / np.maximum(cb, 1e-300) + 1.0 / max(-cpn, 1e-300), 0.0)
        if mode == 4:
            val = base * (np.maximum(g - clamp, 0.0) / g)[..., None]            # :222
            decided &= ~(keep & (np.abs(g - clamp) < 1.0e-4 * clamp))
            kappa = kappa + np.where(keep & (g > clamp), g / np.maximum(g - clamp, 1e-300), 0.0)
            kappa = kappa[..., None] * np.ones(3)
        else:
            ok2 = cl > 0.0 and float(np.dot(pv.fdir, pv.n)) > 0.0               # LambertEval(-w12, fluxDir, n2, rd2), frag:42-50
            record_decided &= not abs(float(np.dot(pv.fdir, pv.n))) < COS_MARGIN and not abs(cl) < COS_MARGIN
            brdf2 = (pv.rd * INV_PI if ok2 else np.zeros(3))
            if np.any(pv.rs != 0.0):
                record_decided &= not bool(_near_cut(np.float64(dp), CUT_GLSL))
                if dp > CUT_GLSL:
                    brdf2 = brdf2 + pv.rs * (pv.e + 2.0) * dp ** pv.e * INV_PI * 0.5
                    kappa = kappa + pv.e / dp; lam = lam + pv.e * abs(math.log2(dp))
            pre = ph.flux * k * inv_n
            x = brdf1 * brdf2 * g[..., None]
            den = brdf2 * g[..., None]
            val = np.where(den != 0.0, pre * np.maximum(x - clamp, 0.0) / np.where(den != 0.0, den, 1.0), 0.0)   # :232; zero channel -> 0
            decided &= ~(keep & np.any(np.abs(x - clamp) < 1.0e-4 * clamp, axis=-1))
            kappa = kappa[..., None] + np.where(keep[..., None] & (x > clamp), x / np.maximum(x - clamp, 1e-300), 0.0)
        val = np.where(keep[..., None], val, 0.0)                               # discard, :219, :229
    if not alive:
        val = np.zeros_like(val)                                                # :235-238
    if kappa.ndim == val.ndim - 1:
        kappa = kappa[..., None] * np.ones(3)
    decided = decided & record_decided
    val = np.where(inside[..., None], val, 0.0)
    return val, kappa, lam, decided, inside, radius_decided


def bar(f64, kappa, lam, K, hw_pow):
    """(K 2^-24 kappa [+ 2^-22 lam]) |f64| + 1e-20, per channel"""
    kappa = kappa if kappa.ndim == f64.ndim else kappa[..., None]
    rel = K * 2.0 ** -24 * kappa + (2.0 ** -22 * lam[..., None] if hw_pow else 0.0)
    return rel * np.abs(f64) + 1.0e-20


def worst_ratio(got, f64, kappa, lam, decided, hw_pow=False):
    """the smallest K under which bar() holds on the decided entries (0 if nothing is compared); the lam term, if any, is granted first"""
    kappa = kappa if kappa.ndim == f64.ndim else kappa[..., None]
    err = np.abs(np.asarray(got, np.float64) - f64) - 1.0e-20 - (2.0 ** -22 * lam[..., None] * np.abs(f64) if hw_pow else 0.0)
    den = 2.0 ** -24 * kappa * np.abs(f64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / den, 0.0)
    ratio = np.where(decided[..., None], ratio, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ the whole domain
class Domain:
    """the inputs, built once per test module, and the float64 answers, computed once per (mode, record)"""

    def __init__(self, oa):
        self.scene = floor_scene()
        self.oracle_scene = oa.Scene(self.scene)
        planes = self.oracle_scene.primary(W, H)
        self.gbuf, self.pixel_names = make_receiver(planes[0], planes[1])
        self.pixel = pixels_of(self.gbuf)
        self.vpls, self.vpl_names = make_vpls()
        self.photons, self.photon_names, self.photon_slots = make_photons(planes[0])
        self._vpl, self._photon = {}, {}

    def coverage(self):
        return coverage(self.pixel_names, self.vpl_names, self.photon_names)

    def vpl_ref(self, mode, k):
        if (mode, k) not in self._vpl:
            self._vpl[mode, k] = vpl_pair_f64(mode, params(mode), self.pixel, self.vpls[k])
        return self._vpl[mode, k]

    def photon_ref(self, mode, k):
        if (mode, k) not in self._photon:
            s = self.photon_slots[k]
            self._photon[mode, k] = photon_frag_f64(mode, params(mode), self.pixel, self.photons[s], self.photons[s - 1])
        return self._photon[mode, k]


def check_caps(undecided_per_record, lit_pairs):
    """the conditions on the inputs: at most 8 undecided pixels per (record, mode), at most 0.5 % of all lit pairs"""
    worst = max(undecided_per_record) if undecided_per_record else 0
    total = sum(undecided_per_record)
    assert worst <= 8, f"{worst} undecided pixels under one record"
    assert total <= 0.005 * lit_pairs, f"{total} undecided of {lit_pairs} lit pairs"
    return worst, total
