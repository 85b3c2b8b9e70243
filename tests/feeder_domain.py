"""Inputs that visit every arm of the two feeder kernels, and their float64 restatement (numpy only; the oracle serves once, for the
receiver's primary G-buffer, as in shading_domain.Domain).

light_trace_kernel (kernels_trace.hip <- tracePhotons + rtMaterialClosestHit, rt/lighttracing.cu:192-250, 113-182) is restated VERTEX BY
VERTEX, teacher-forced from the records under test: record i as written (float32 taken as reals) and the position in the path's stream,
which follows from the flags, give record i + 1 in float64.  Errors do not compound, so every field has a bar of a few 2^-24.
path_trace_pixel (pt_common.hpp <- pathTraceSimple + its closest-hit program, rt/pathtracing.cu:240-348, 112-228) shows only the radiance,
so it is restated whole, per pixel, with the terms the value is the sum of (one next-event term per vertex, the emitter hit) and a
conditioning number per term.  Quirks of the reference that are kept (and where they are):
  * russianProb of the path tracer is a MAX with 0.98 (pathtracing.cu:55), of light tracing a min (lighttracing.cu:93-96).
  * LambertSample is taken about the geometric normal at bounces (pathtracing.cu:197) and about the G-buffer normal at the first vertex;
    PhongSample of light tracing about the un-flipped normal (lighttracing.cu:176).  Back faces end a path before either is used.
  * PhongEvalF has no reflectance test (rtmaterial.cuh:112-118); PhongEval and PhongPdfA test rho_s.x alone against 1e-6 (:104-110, :92).
  * LambertPdfA carries 1 / pi (rtmaterial.cuh:53); GeometryTerm and LambertPdfA take the UNNORMALISED v12 (:30-38, :46-54).
  * stored flux is the flux BEFORE the division by the roulette probability (lighttracing.cu:164-166); the last slot of a path still draws
    and samples, and carries the lobe bit.
  * a miss, a back face, an emitter and a black material end a light path without a record (no miss program; :124-128, :143-147).
Ray casting is brute force over all triangles with optix::intersect_triangle_branchless (rt/triangleintersect.cu:17-41): tmin 1e-4 in light
tracing; tmin 1e-5 with shadow segments [1e-4, 1 - 1e-4] at the first vertex and [1e-5, 0.99999] at bounces in the path tracer; the light's
triangles are hit like any other.

Every evaluation says how well conditioned it is (kappa, in the sense of shading_domain: e / d per lobe power, 1 / cos per cosine that
is a difference, the MIS weight's share of its pdf's error, the sampled direction's error in units of 2^-24 -- shading_domain._lambert_local /
_phong_local -- where a cosine or a hit point is taken with it) and whether it is DECIDED: False where a discrete comparison lies within
its margin.  The margins, next to what they come from:
  COS_MARGIN 4e-6    a clamped cosine, a lobe cosine against 0 and against the cut 1e-6, dot(gn, dir) against 0 (shading_domain's)
  SEL_ULPS   8       choose against psel: psel = ml / (mp + ml) of float32 reflectances has two roundings (1.5 2^-24 relative), of texels
                     the fetch's (kappa_tex) on top; the draws are exact
  RR_ULPS    8       the roulette draw against russian: exact in light tracing (a max / min of recorded numbers), att's roundings in the
                     path tracer (att_kappa on top)
  BLACK      1e-7    max_l + max_p against 1e-6
  CDF_MARGIN 1e-6    a CDF entry (a float32 running sum divided by its total: 3 roundings of numbers <= 1) against r
  EDGE       1e-4    barycentric distance of a hit to an edge of its triangle: a relative 1e-4 of the patch size, two orders above what the
                     sampled direction's error (6 - 60 units of 2^-24 of the distance) moves a hit by
  T_REL      1e-4    a runner-up within this relative distance in t
  tmin, tmax         a hit within tmin / 2 of either end of the segment, or within what t is uncertain by for a grazing ray: 3 2^-24 of the
                     end point's coordinates over the cosine to the plane (cast())
  FLOOR      1e-5    u w - 0.5 within this of an integer (the texel pair changes)
  p.z exactly 0      of a sampled direction (the lobe bit is set, the weight is 0)
A sample that is not decided is compared with nothing.
"""
import math
from collections import Counter
from types import SimpleNamespace

import numpy as np

import shading_domain as sd

W, H = sd.W, sd.H
E_SET = sd.E_SET
BIG = sd.BIG
COS_MARGIN = sd.COS_MARGIN
CUT = sd.CUT_CUDA
INV_PI = sd.INV_PI
ULP = sd.ULP
SEL_ULPS = 8.0
RR_ULPS = 8.0
BLACK = float(np.float32(0.000001))
BLACK_MARGIN = 1.0e-7
CDF_MARGIN = 1.0e-6
EDGE = 1.0e-4
T_REL = 1.0e-4
FLOOR_MARGIN = 1.0e-5
POINT_ULPS = 3.0
CHOOSE_MAX = float(np.float32(0.999999))
RR_LT = float(np.float32(0.98))
LIGHT_EXPONENTS = (0.0, 5.0)
LT_P = (2, 4, 7)
LT_PATHS = 200
LT_SEEDS = (104, 0x9E3779CD)        # of the seeds tried, two under which the light's small triangle is drawn 5 and 6 times in 200 paths; the second has bit 31 set
PT_SEEDS = (3, 4)
PT_BOUNCES = (1, 2, 3)
PT_SUBSTREAM = 0x50540000
USABLE_VPL, USABLE_PHOTON, LAMBERT_ONLY, PHONG_ONLY = 1, 2, 4, 8

CLASSES = ("lambert_e_left", "rsx_zero", "rsx_tiny", "pure_spec", "textured") + tuple(f"e_{e:g}" for e in E_SET)


# ------------------------------------------------------------------------------------------------------------------ the patch room
SCALE = 0.125                   # of every length below: what a grazing ray's t is uncertain by against tmin = 1e-5 grows with the coordinates
Z0 = 5.0 * SCALE              # the light's height over the floor.  The LIGHT's plane is z = 0 and the floor z = -Z0 (both exact in float32): a shadow
                              # ray leaves a light sample whose z is exact, so a grazing one knows on which side of tmin the light's own plane lies;
                              # with the light at z = Z0, 1.8 % of the room's height under it was undecided for that reason alone
CAMERA = (0.0, 0.0, 10.0 * SCALE - Z0)


def receiver_floor():
    """shading_domain.floor_scene at this module's scale: the floor z = 0 under the whole frame, seen straight down from 10 SCALE (Domain
    moves the positions it gives to z = -Z0)"""
    import scenes
    s = scenes.SceneData()
    s.aspect = W / H
    s.add_quad([-12.0 * SCALE, -8.0 * SCALE, 0.0], [24.0 * SCALE, 0.0, 0.0], [0.0, 16.0 * SCALE, 0.0], s.add_material((0.5, 0.5, 0.5)))
    lm = s.add_material((0, 0, 0))
    s.light_mesh = s.add_quad([-0.5, -0.5, 90.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], lm)
    s.light_intensity = [1.0, 1.0, 1.0, 0.0]
    s.cam_origin = [0.0, 0.0, 10.0 * SCALE]; s.cam_lookat = [0.0, 0.0, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.fovy = sd.FOVY
    s.triangle_soup()
    return s


def patch_room(light_exponent):
    """SCALE times [-10, 10] x [-7, 7] x [0, 5.1], moved down by Z0: 8 floor patches, 14 wall patches, 2 ceiling patches over x < 4 (the rest is open: rays
    leave), one box floating under the light, a light of three triangles (areas 2 : 1 : 0.02) under the ceiling, facing down.  Every patch
    has a material of its own; s.patch_class[material] names its class."""
    import scenes
    s = scenes.SceneData()
    s.aspect = W / H
    rng = np.random.RandomState(20264)
    s.patch_class = {}
    tex_kd = np.zeros((3, 5, 4), np.float32); tex_kd[..., :3] = 0.15 + 0.7 * rng.rand(3, 5, 3)
    tex_ks = np.zeros((1, 1, 4), np.float32); tex_ks[0, 0, :3] = (0.3, 0.2, 0.25)
    tex_ns = np.zeros((3, 5, 4), np.float32); tex_ns[..., 0] = 1.0 + 30.0 * rng.rand(3, 5)
    s.textures += [tex_kd, tex_ks, tex_ns]

    def mat(cls):
        rd = 0.2 + 0.6 * rng.rand(3); rs = 0.1 + 0.4 * rng.rand(3)
        if cls == "lambert_e_left":
            m = s.add_material(rd, (0, 0, 0), 37.0)
        elif cls.startswith("e_"):
            m = s.add_material(rd, rs, float(cls[2:]))
        elif cls == "rsx_zero":
            m = s.add_material(rd, (0.0, rs[1], rs[2]), 20.0)
        elif cls == "rsx_tiny":
            m = s.add_material(rd, (5.0e-7, rs[1], rs[2]), 20.0)
        elif cls == "pure_spec":
            m = s.add_material((0, 0, 0), 0.5 + rs, 20.0)
        elif cls == "black":
            m = s.add_material((2.0e-7, 0.0, 1.0e-7), (0.0, 3.0e-7, 0.0), 5.0)
        elif cls == "back":
            m = s.add_material(rd)
        elif cls == "textured":
            m = s.add_material((9.0, 9.0, 9.0), (9.0, 9.0, 9.0), 9.0, tex_kd=0, tex_ks=1, tex_ns=2)     # (every constant is replaced by a texel)
        s.patch_class[m] = cls
        return m

    def patch(o, u, v, cls):
        o, u, v = (np.asarray(a, np.float64) * SCALE for a in (o, u, v))
        o = o - [0.0, 0.0, Z0]
        m = mat(cls)
        if cls == "back":
            u, v = v, u                                                # reversed winding: the normal points out of the room
        if cls == "textured":                                          # corner uv from below 0 to above 1 in both directions
            s.add_mesh([o, o + u, o + u + v, o + v], [(0, 1, 2), (0, 2, 3)], m, [(-0.3, -0.4), (1.4, -0.4), (1.4, 1.5), (-0.3, 1.5)])
        else:
            s.add_quad(o, u, v, m)

    floor = ["lambert_e_left", "e_0.5", "e_20", "textured", "rsx_zero", "e_1000", "pure_spec", "rsx_tiny"]
    for k, cls in enumerate(floor):
        patch([-10.0 + 5.0 * (k % 4), -7.0 + 7.0 * (k // 4), 0.0], [5.0, 0, 0], [0, 7.0, 0], cls)
    wx = ["e_0", "black", "lambert_e_left", "textured", "back", "e_200"]
    for k, cls in enumerate(wx):                                       # x = -10 (normal +x) and x = 10 (normal -x), three patches each
        y0 = -7.0 + 14.0 / 3.0 * (k % 3)
        if k < 3:
            patch([-10.0, y0, 0.0], [0, 14.0 / 3.0, 0], [0, 0, 5.1], cls)
        else:
            patch([10.0, y0, 0.0], [0, 0, 5.1], [0, 14.0 / 3.0, 0], cls)
    wy = ["e_1", "rsx_tiny", "pure_spec", "e_1000", "rsx_zero", "e_0.5", "e_20", "lambert_e_left"]
    for k, cls in enumerate(wy):                                       # y = -7 (normal +y) and y = 7 (normal -y), four patches each
        x0 = -10.0 + 5.0 * (k % 4)
        if k < 4:
            patch([x0, -7.0, 0.0], [0, 0, 5.1], [5.0, 0, 0], cls)
        else:
            patch([x0, 7.0, 0.0], [5.0, 0, 0], [0, 0, 5.1], cls)
    patch([-10.0, -7.0, 5.1], [0, 14.0, 0], [7.0, 0, 0], "e_200")     # ceiling, normal -z
    patch([-3.0, -7.0, 5.1], [0, 14.0, 0], [7.0, 0, 0], "e_0")
    box = mat("lambert_e_left")
    s.add_box(np.array([-3.0, -2.0, 2.0]) * SCALE - [0, 0, Z0], np.array([0.0, 1.0, 3.0]) * SCALE - [0, 0, Z0], box, True, 1)        # the occluder: under the light's large triangle
    lm = s.add_material((0, 0, 0))
    s.patch_class[lm] = "light"
    z = 5.0
    lv = [[-2.0, -1.0, z], [-2.0, 1.0, z], [0.0, -1.0, z],             # area 2
          [0.5, -1.0, z], [0.5, 0.0, z], [2.5, -1.0, z],               # area 1
          [0.5, 0.5, z], [0.5, 0.7, z], [0.7, 0.5, z]]                 # area 0.02: 0.66 % of 3.02
    s.light_mesh = s.add_mesh(np.array(lv) * SCALE - [0, 0, Z0], np.arange(9).reshape(3, 3), lm)
    s.light_intensity = [3.0, 2.5, 2.0, float(light_exponent)]
    # the scene's own camera serves the batched path tracer alone, which draws its own G-buffer: inside the room, under the open part of the
    # ceiling, looking at the floor, two walls, the box and the light.  Every other case uploads the receiver and names CAMERA as the eye.
    s.cam_origin = [8.0 * SCALE, -1.0 * SCALE, 4.0 * SCALE - Z0]; s.cam_lookat = [-3.0 * SCALE, 0.5 * SCALE, 0.5 * SCALE - Z0]; s.cam_up = [0.0, 0.0, 1.0]
    s.fovy = sd.FOVY
    s.triangle_soup()
    return s


class Geometry:
    """the scene's float32 numbers as float64 arrays"""

    def __init__(self, s):
        verts, uvs, mat = s.triangle_soup()
        v = verts.astype(np.float64).reshape(-1, 3, 3)
        self.p0, self.p1, self.p2 = v[:, 0], v[:, 1], v[:, 2]
        self.e0 = self.p1 - self.p0; self.e1 = self.p0 - self.p2
        self.n = np.cross(self.e1, self.e0)                             # triangleintersect.cu:31 (unnormalised)
        self.gn = self.n / np.sqrt((self.n * self.n).sum(-1))[:, None]
        self.uv = uvs.astype(np.float64)
        self.mat = mat
        f = lambda x: np.asarray(x, np.float32).astype(np.float64)
        self.kd = [f(m["kd"]) for m in s.materials]; self.ks = [f(m["ks"]) for m in s.materials]; self.ns = [float(np.float32(m["ns"])) for m in s.materials]
        self.tex = [(m["tex_kd"], m["tex_ks"], m["tex_ns"]) for m in s.materials]
        self.textures = [np.asarray(t, np.float32).astype(np.float64) for t in s.textures]
        self.cls = [s.patch_class[m] for m in range(len(s.materials))]
        self.light_first, self.light_count = s.light_first, s.light_count
        self.is_light = np.array([s.patch_class[m] == "light" for m in mat])
        I = f(s.light_intensity)
        self.lw = float(I[3])
        self.li = I[:3] * math.pi                                        # rtcommon.h:780-782: xyz scaled by pi
        lt = slice(s.light_first, s.light_first + s.light_count)
        c = np.cross(self.p1[lt] - self.p0[lt], self.p2[lt] - self.p0[lt])
        areas = 0.5 * np.sqrt((c * c).sum(-1))
        self.light_area = float(areas.sum())
        self.cdf = np.cumsum(areas) / self.light_area                    # rtcommon.h:501-531
        self.cdf[-1] = 1.0


def cast(G, o, d):
    den = G.n @ d
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (G.p0 - o) / den[:, None]
        i = np.cross(d, q)
        beta = (i * G.e1).sum(-1); gamma = (i * G.e0).sum(-1); t = (G.n * q).sum(-1)
    ok = np.isfinite(t) & np.isfinite(beta) & np.isfinite(gamma)
    inside = ok & (beta > EDGE) & (gamma > EDGE) & (beta + gamma < 1.0 - EDGE)
    amb = ok & ~inside & (beta > -EDGE) & (gamma > -EDGE) & (beta + gamma < 1.0 + EDGE)
    # what t is uncertain by in float32: the ray's origin is a computed point (a light sample is a sum of three products, a hit is o + d t:
    # up to POINT_ULPS = 3 roundings of numbers no larger than the coordinate), coordinate k within 3 2^-24 |o_k| of where it should be, and
    # t = n . (p0 - o) / (n . d) turns that into 3 2^-24 sum |n_k| |o_k| / |n . d| (for the far end of a segment, that point's coordinates on top): a grazing ray
    # cannot tell on which side of tmin / tmax a plane through one of its ends lies (a point of the plane z = 0 is exact, and so is its t)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = POINT_ULPS * ULP * (np.abs(G.n) @ np.abs(o)) / np.abs(den)
        tol_end = tol + POINT_ULPS * ULP * (np.abs(G.n) @ np.abs(o + d)) / np.abs(den)     # (of a segment's far end o + d, a computed point too)
    tol = np.where(np.isfinite(tol), tol, np.inf); tol_end = np.where(np.isfinite(tol_end), tol_end, np.inf)
    # an origin whose coordinate IS an axis-aligned plane's (a receiver pixel of the floor, a light sample of the light's plane) gives
    # p0 - o = 0 along the normal and t = 0 in float32 as here: nothing is uncertain
    tol = np.where((t == 0.0) & ((G.n != 0.0).sum(-1) == 1), 0.0, tol)
    return t, beta, gamma, inside, amb, tol, tol_end


def closest(G, o, d, tmin):
    """(triangle or -1, t, beta, gamma, decided)"""
    t, beta, gamma, inside, amb, tol, _ = cast(G, o, d)
    cand = inside & (t > tmin)
    m = np.maximum(0.5 * tmin, tol)
    decided = not np.any(inside & (np.abs(t - tmin) < m))
    if not cand.any():
        decided &= not np.any(amb & (t > tmin - m))
        return -1, math.inf, 0.0, 0.0, decided
    k = int(np.argmin(np.where(cand, t, np.inf)))
    lim = t[k] * (1.0 + T_REL)
    decided &= not np.any(amb & (t > tmin - m) & (t < lim))
    other = cand.copy(); other[k] = False
    decided &= not np.any(other & (t < lim))
    return k, float(t[k]), float(beta[k]), float(gamma[k]), decided


def occluded(G, o, d, tmin, tmax):
    """(occluded, decided): any triangle with t in (tmin, tmax) of the segment o + t d"""
    t, beta, gamma, inside, amb, tol, tol_end = cast(G, o, d)
    m, m_end = np.maximum(0.5 * tmin, tol), np.maximum(0.5 * tmin, tol_end)
    hit = bool(np.any(inside & (t > tmin) & (t < tmax)))
    decided = not np.any(amb & (t > tmin - m) & (t < tmax + m_end)) and not np.any(inside & ((np.abs(t - tmin) < m) | (np.abs(t - tmax) < m_end)))
    return hit, decided


# ------------------------------------------------------------------------------------------------------------------ RNG
_M64 = (1 << 64) - 1


def stream(index, seq, sub):
    """splitmix64-seeded PCG32 XSH-RR in Python integers (device_common.hpp rng_init / rng_u32): a function that returns the next 32 bits"""
    s0 = sd.splitmix64((((seq << 32) | index) + sub * 0xD1B54A32D192ED03) & _M64)
    inc = sd.splitmix64(s0) | 1
    st = [(s0 + inc) & _M64]

    def u32():
        old = st[0]
        st[0] = (old * 6364136223846793005 + inc) & _M64
        xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
        rot = old >> 59
        return ((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF
    u32()
    return u32


def uniforms(index, seq, sub):
    """the next uniform, (k + 1) 2^-24: exact in float32 and in float64"""
    u32 = stream(index, seq, sub)
    return lambda: ((u32() >> 8) + 1) / 16777216.0


# ------------------------------------------------------------------------------------------------------------------ shared helpers
def _unit(v):
    return v / math.sqrt(float(v @ v))


def _mirror(v, n):
    return 2.0 * n * float(n @ v) - v


def _frame_dir(n, p):
    t, b, nn, tie = sd._onb(n)
    tie = bool(tie) and not (n[0] == 0.0 and n[2] == 0.0)               # (a wall's normal along y: |0| > |0| is false for everyone)
    return t * p[0] + b * p[1] + nn * p[2], tie


def _near_cut(d):
    return abs(d) < COS_MARGIN or abs(d - CUT) < COS_MARGIN


def _tex2d(tex, u, v):
    """tex2D, linear / repeat / normalised (rtcommon.h:223-245): (rgba, spread per channel of the texels mixed, decided)"""
    h, w = tex.shape[:2]
    if w == 1 and h == 1:
        return tex[0, 0], np.zeros(4), True
    xb, yb = u * w - 0.5, v * h - 0.5
    xf, yf = math.floor(xb), math.floor(yb)
    a, b = xb - xf, yb - yf
    decided = abs(xb - round(xb)) > FLOOR_MARGIN and abs(yb - round(yb)) > FLOOR_MARGIN
    x0, x1, y0, y1 = int(xf) % w, (int(xf) + 1) % w, int(yf) % h, (int(yf) + 1) % h
    px = np.stack([tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]])
    r = (1 - a) * (1 - b) * px[0] + a * (1 - b) * px[1] + (1 - a) * b * px[2] + a * b * px[3]
    return r, px.max(0) - px.min(0), decided


def material_at(G, tri, beta, gamma, cov=None):
    """(kd, ks, ns, kappa_tex, decided, textured): kappa_tex = the fetch's error in units of 2^-24 of the result -- u and v are sums of
    three products of corner coordinates up to 1.5 (6 units), scaled by the texture's size, times the spread of the four texels"""
    m = int(G.mat[tri])
    kd, ks, ns = G.kd[m], G.ks[m], G.ns[m]
    tk, ts, tn = G.tex[m]
    if tk < 0 and ts < 0 and tn < 0:
        return kd, ks, ns, 0.0, True, False
    uv = G.uv[tri]
    w0 = 1.0 - beta - gamma
    u = uv[2] * beta + uv[4] * gamma + uv[0] * w0
    v = uv[3] * beta + uv[5] * gamma + uv[1] * w0
    if cov is not None:
        cov["tex_u_below_0" if u < 0 else "tex_u_above_1" if u > 1 else "tex_u_inside"] += 1
        cov["tex_v_below_0" if v < 0 else "tex_v_above_1" if v > 1 else "tex_v_inside"] += 1
    kappa, decided = 0.0, True
    out = []
    for t, const in ((tk, kd), (ts, ks), (tn, ns)):
        if t < 0:
            out.append(const); continue
        tex = G.textures[t]
        c, spread, dec = _tex2d(tex, u, v)
        decided &= dec
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(spread[:3] > 0, 8.0 * (tex.shape[0] + tex.shape[1]) * spread[:3] / np.maximum(np.abs(c[:3]), 1e-300), 0.0)
        kappa = max(kappa, float(k.max() if const is not ns else k[0]))
        out.append(c)
    return out[0][:3], out[1][:3], (float(out[2][0]) if tn >= 0 else out[2]), 4.0 + kappa, decided, True


def class_of(ks, ns, kd, textured):
    if textured:
        return "textured"
    if not np.any(ks != 0.0):
        return "lambert_e_left"
    if not np.any(kd != 0.0):
        return "pure_spec"
    if ks[0] == 0.0:
        return "rsx_zero"
    if ks[0] < 1.0e-6:
        return "rsx_tiny"
    return f"e_{ns:g}"


def light_sample(G, u, cov, perturb=None):
    """LightSample (rtlightsource.cuh:24-80): (triangle, position, normal, decided)"""
    r = u()
    k = int(np.searchsorted(G.cdf, r, side="left"))                  # the first entry that is not < r
    k = min(k, G.light_count - 1)
    decided = not np.any(np.abs(G.cdf[:-1] - r) < CDF_MARGIN)
    x = u(); y = u()
    sq = math.sqrt(x); beta = sq * (1.0 - y); gamma = sq * y
    if perturb == "swap_beta_gamma":
        beta, gamma = gamma, beta
    t = G.light_first + k
    p1, p2, p3 = G.p0[t], G.p1[t], G.p2[t]
    pos = p1 * beta + p2 * gamma + p3 * (1.0 - gamma - beta)
    n = _unit(np.cross(p2 - p1, p3 - p1))
    cov[f"light_triangle_{k}"] += 1
    return k, pos, n, decided


def sample_lambert(u, n):
    """LambertSample (rtmaterial.cuh:56-66): (direction, its absolute error in units of 2^-24, cos, decided)"""
    u1 = u(); u2 = u()
    p, err = sd._lambert_local(np.float64(u1), np.float64(u2))
    d, tie = _frame_dir(n, p)
    return d, float(err) / ULP, float(p[2]), (not tie) and p[2] != 0.0


def sample_phong(u, in_dir, n, e, in_err=0.0):
    """PhongSample (rtmaterial.cuh:120-154) about reflect(-in, n): (direction, error in units of 2^-24, unsafe cos to n, cos to r, decided).
    in_err: what in_dir is off by, in the same units -- the mirror hands it on to the sample"""
    r = _mirror(in_dir, n)
    sx = u(); sy = u()
    p, err = sd._phong_local(e, np.float64(sx), np.float64(sy))
    d, tie = _frame_dir(r, p)
    unsafe = float(d @ n)
    return d, float(err) / ULP + in_err, unsafe, float(p[2]), (not tie) and abs(unsafe) >= COS_MARGIN + in_err * ULP


# ------------------------------------------------------------------------------------------------------------------ light tracing
class Compare:
    """collects error / (2^-24 kappa scale) of every comparison made and the exact mismatches"""

    def __init__(self):
        self.worst = 0.0; self.worst_what = ""; self.exact = []; self.count = 0

    def near(self, what, got, want, kappa, scale=None):
        got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
        sc = np.abs(want) if scale is None else scale
        err = np.abs(got - want) - 1.0e-20
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0.0, err / (ULP * kappa * sc), 0.0)
        r = float(np.max(r))
        self.count += 1
        if not r <= self.worst:                                        # (a NaN counts)
            self.worst, self.worst_what = (r if r == r else math.inf), f"{what}: got {got.tolist()}, float64 {want.tolist()}, kappa {kappa:.3g}"

    def same(self, what, got, want):
        self.count += 1
        if not np.array_equal(np.asarray(got), np.asarray(want)):
            self.exact.append(f"{what}: got {np.asarray(got).tolist()}, expected {np.asarray(want).tolist()}")


def _zero_tail(cmp, rec, i, what):
    tail = rec[i:]
    cmp.same(f"{what}: slots {i}.. after the end are all zero", bool(tail.size == 0 or not np.any(np.frombuffer(tail.tobytes(), np.uint8))), True)


def light_path_f64(G, rec, path_id, seed, cmp, cov, perturb=None):
    """one light path's P records against float64, vertex by vertex.  Returns True if every vertex was decided; an undecided vertex ends the
    walk (what follows it is compared with nothing)."""
    P = rec.shape[0]
    what = f"path {path_id}"
    u = uniforms(path_id, seed, 0)
    f64 = lambda a: np.asarray(a, np.float64)
    k, pos, n, decided = light_sample(G, u, cov, perturb)
    if not decided:
        return False
    # the emission direction: PhongSample about the normal with the light's exponent and reflectance 1 (lighttracing.cu:208-213)
    d, derr, unsafe, cos_r, dec = sample_phong(u, n, n, G.lw)
    r0 = rec[0]
    tl = G.light_first + k
    scale_pos = float(max(np.abs(G.p0[tl]).max(), np.abs(G.p1[tl]).max(), np.abs(G.p2[tl]).max()))     # (a sum of three corners times weights: the corners' size)
    cmp.near(what + " on-light position", r0["pos"], pos, 4.0, scale_pos)
    cmp.near(what + " on-light normal", r0["normal"], n, 4.0, 1.0)
    cmp.near(what + " on-light flux", r0["flux"], G.li * G.light_area, 4.0)
    cmp.same(what + " record 0 constants", [int(r0["flags"]), float(r0["p_select_lambert"]), float(r0["phong_exp"])] + r0["rho_d"].tolist() + r0["rho_s"].tolist(),
             [USABLE_VPL, 0.0, G.lw, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
    cmp.same(what + " record 0 flux_dir is its normal", r0["flux_dir"].tobytes(), r0["normal"].tobytes())
    if not dec:
        return False
    carry = f64(r0["flux"]) * ((G.lw + 2.0) / (G.lw + 1.0) * max(unsafe, 0.0))     # flux * att
    carry_kappa = 4.0 + derr / max(unsafe, 1e-300)
    origin = f64(r0["pos"])
    for i in range(1, P):
        r = rec[i]
        present = int(r["flags"]) != 0
        if present:
            used = -f64(r["flux_dir"])                                  # the direction that left vertex i - 1, as the device took it
            cmp.near(f"{what} direction leaving vertex {i - 1}", used, d, 4.0 + derr, 1.0)
        else:
            used = d
        tri, t, beta, gamma, dec = closest(G, origin, used, 1.0e-4)
        if not dec:
            return False
        end = None
        if tri < 0:
            end = "miss"
        else:
            front = float(G.gn[tri] @ used)
            if abs(front) < COS_MARGIN:
                return False
            if front > 0.0:
                end = "back_face"
            elif G.is_light[tri]:
                end = "emitter"
            else:
                kd, ks, ns, ktex, dec, textured = material_at(G, tri, beta, gamma, cov)
                if not dec:
                    return False
                ml, mp = float(kd.max()), float(ks.max())
                if abs(ml + mp - BLACK) < BLACK_MARGIN:
                    return False
                if ml + mp <= BLACK:
                    end = "black"
        if end:
            cov["lt_end_" + end] += 1; cov[f"lt_ends_after_slot_{i - 1}"] += 1
            _zero_tail(cmp, rec, i, f"{what} ({end} after vertex {i - 1})")
            return True
        cls = class_of(ks, ns, kd, textured)
        cov[("lt_first:" if i == 1 else "lt_bounce:") + cls] += 1
        if not present:
            cmp.same(f"{what} vertex {i} ({cls}) has no record", 0, 1)
            return True
        hit = origin + used * t
        psel = ml / (mp + ml)
        choose = min(u(), CHOOSE_MAX)
        stored = carry
        if perturb == "flux_after_division":
            stored = carry / min(float(carry.max()), RR_LT)
        # what the record holds
        cmp.near(f"{what} vertex {i} position", r["pos"], hit, 4.0, float(np.abs(origin).max()) + t)
        cmp.near(f"{what} vertex {i} normal", r["normal"], G.gn[tri], 4.0, 1.0)
        cmp.near(f"{what} vertex {i} psel", r["p_select_lambert"], psel, 4.0 + 2.0 * ktex)
        cmp.near(f"{what} vertex {i} flux", r["flux"], stored, carry_kappa)
        if textured:
            cmp.near(f"{what} vertex {i} kd (texels)", r["rho_d"], kd, ktex); cmp.near(f"{what} vertex {i} ks (texels)", r["rho_s"], ks, ktex)
            cmp.near(f"{what} vertex {i} ns (texel)", r["phong_exp"], ns, ktex)
        else:                                                           # the triangle's material, bit for bit
            cmp.same(f"{what} vertex {i} material", r["rho_d"].tolist() + r["rho_s"].tolist() + [float(r["phong_exp"])], kd.tolist() + ks.tolist() + [ns])
        # the decisions, on the record's own numbers (teacher forcing)
        rflux, rpsel = f64(r["flux"]), float(r["p_select_lambert"])
        russian = min(float(rflux.max()), RR_LT)                        # lighttracing.cu:93-96, :164
        draw = u()
        if abs(choose - rpsel) < SEL_ULPS * ULP * (1.0 + ktex) or abs(draw - russian) < RR_ULPS * ULP * russian:
            return False
        done = draw >= russian                                          # :166
        flag = (USABLE_VPL | USABLE_PHOTON) if i != P - 1 else USABLE_PHOTON
        rn, rin = f64(r["normal"]), f64(r["flux_dir"])
        rkd, rks, rns = f64(r["rho_d"]), f64(r["rho_s"]), float(r["phong_exp"])
        if not done:
            cov["lt_roulette_survived"] += 1
            if choose < rpsel:
                d, derr, cosn, dec = sample_lambert(u, rn)
                w = rkd / rpsel; wk = 0.0
                flag |= LAMBERT_ONLY; cov["lt_lobe_lambert"] += 1
            else:
                d, derr, unsafe, cos_r, dec = sample_phong(u, rin, rn, rns)
                w = rks * ((rns + 2.0) / (rns + 1.0) * max(unsafe, 0.0)) / (1.0 - rpsel)
                wk = derr / unsafe if unsafe > 0.0 else 0.0
                flag |= PHONG_ONLY; cov["lt_lobe_phong"] += 1
            if not dec:
                cmp.same(f"{what} vertex {i} flags", int(r["flags"]), flag)
                return False
            carry = rflux / russian * w
            carry_kappa = 6.0 + wk
        else:
            cov["lt_roulette_ended"] += 1
        cmp.same(f"{what} vertex {i} flags", int(r["flags"]), flag)
        if done:
            cov[f"lt_ends_after_slot_{i}"] += 1
            _zero_tail(cmp, rec, i + 1, f"{what} (roulette at vertex {i})")
            return True
        origin = f64(r["pos"])
    cov[f"lt_ends_after_slot_{P - 1}"] += 1
    return True


def check_light_paths(G, records, seed, P, begin=0, perturb=None):
    """every path of `records` ([n * P], path `begin` first) against float64.  Returns a namespace: worst (error / (2^-24 kappa scale)),
    worst_what, exact (mismatches of what is compared exactly), undecided (paths), paths, coverage (Counter), compared"""
    cmp, cov = Compare(), Counter()
    n = records.shape[0] // P
    und = 0
    for k in range(n):
        und += not light_path_f64(G, records[k * P:(k + 1) * P], begin + k, seed, cmp, cov, perturb)
    return SimpleNamespace(worst=cmp.worst, worst_what=cmp.worst_what, exact=cmp.exact, undecided=und, paths=n, coverage=cov, compared=cmp.count)


# ------------------------------------------------------------------------------------------------------------------ path tracer
def _nee(G, n1, lobe, rho, e, back, lp, ln, point, att, att_k, pos_err, sel, out, back_err=2.0):
    """the next-event term of one vertex if nothing occludes it (pathtracing.cu:262-289, :176-215).  Returns (decided, (term [3], kappa)
    or None where the term is zero whatever the shadow ray says)."""
    to_light = lp - point
    d2 = float(to_light @ to_light); dist = math.sqrt(d2)
    tln = to_light / dist
    cos1, cos2 = float(n1 @ tln), -float(ln @ tln)
    m = COS_MARGIN + pos_err * ULP / dist
    if abs(cos1) < m or abs(cos2) < m:
        return False, None
    if cos1 <= 0.0 or cos2 <= 0.0:
        out.cov["nee_zero_geometry"] += 1
        return True, None
    g = cos1 * cos2 / d2                                                # GeometryTerm on the unnormalised v12: c1 c2 / d2^2
    kappa = 4.0 + 1.0 / cos1 + 1.0 / cos2 + att_k
    disp = pos_err / dist * (2.0 + 1.0 / cos1 + 1.0 / cos2)
    # PhongEvalF(ln, -tln, ln, lw): the light's emission lobe, cosine = cos2
    if G.lw != 0.0 and _near_cut(cos2):
        return False, None
    if cos2 <= CUT:
        return True, None
    fl = (G.lw + 2.0) * cos2 ** G.lw * INV_PI * 0.5
    kappa += G.lw / cos2; disp += pos_err / dist * G.lw / cos2
    lpdf = 1.0 / G.light_area
    if lobe == "L":
        bpdf = g * INV_PI                                               # LambertPdfA carries 1 / pi
        f = rho * INV_PI
    else:
        c = float(tln @ _mirror(back, n1))                              # PhongPdfA's and PhongEval's cosine (the same number)
        if np.any(rho != 0.0) and _near_cut(c):
            return False, None
        on = c > CUT and rho[0] > CUT                                   # rho_s.x alone
        bpdf = (e + 1.0) * 0.5 * INV_PI * c ** e * cos2 / d2 if on else 0.0
        f = rho * ((e + 2.0) * c ** e * INV_PI * 0.5) if on else np.zeros(3)
        if on:
            kappa += e / c * (1.0 + bpdf / (lpdf + bpdf)); disp += (pos_err / dist + back_err) * e / c * 2.0      # (back is a computed direction too)
    w = lpdf / (lpdf + bpdf)
    term = G.li * G.light_area * w * f * g * att / sel * fl
    if not np.any(term != 0.0):
        return True, None
    return True, (term, kappa + disp)


def path_pixel_f64(G, x, y, first_pos, first_n, rd1, rs1, e1, cam, seed, max_bounces, first_cls=None):
    """path_trace_pixel of one pixel in float64.  Returns a namespace: value [3], terms [(term [3], kappa)], decided, rays, cov (Counter)"""
    out = SimpleNamespace(terms=[], cov=Counter(), decided=False, rays=0, value=np.zeros(3))
    cov = out.cov
    u = uniforms(y * W + x, seed, PT_SUBSTREAM)                          # pathtracing.cu:369-370

    def finish(decided=True):
        out.decided = decided
        out.value = sum((t for t, _ in out.terms), np.zeros(3))
        return out

    def add_nee(n1, lobe, rho, e, back, lp, ln, point, att, att_k, pos_err, sel, hit, occ_decided, back_err=2.0):
        """the vertex's next-event term; the shadow ray's answer matters only where the term it gates is not zero anyway"""
        ok, term = _nee(G, n1, lobe, rho, e, back, lp, ln, point, att, att_k, pos_err, sel, out, back_err)
        if not ok or (term is not None and not occ_decided):
            return False
        if term is not None:
            cov["nee_occluded" if hit else "nee_unoccluded"] += 1
            if not hit:
                out.terms.append(term); cov["nee_lit_" + ("lambert" if lobe == "L" else "phong")] += 1
        return True
    camera_vec = _unit(first_pos - cam)
    # the first vertex, from the G-buffer (:246-300)
    k, lp, ln, dec = light_sample(G, u, cov)
    if not dec:
        return finish(False)
    hit, occ_dec = occluded(G, lp, first_pos - lp, 1.0e-4, 1.0 - 1.0e-4); out.rays += 1
    ml, mp = float(rd1.max()), float(rs1.max())
    if abs(ml + mp - BLACK) < BLACK_MARGIN:
        return finish(False)
    if ml + mp <= BLACK:
        cov["pt_first_black"] += 1
        return finish()
    if first_cls:
        cov["pt_first:" + first_cls] += 1
    psel = ml / (mp + ml)
    choose = min(u(), CHOOSE_MAX)
    if abs(choose - psel) < SEL_ULPS * ULP:
        return finish(False)
    att = np.ones(3); att_k = 0.0; pos_err = 0.0
    back = -camera_vec
    if choose < psel:
        if not add_nee(first_n, "L", rd1, e1, back, lp, ln, first_pos, att, att_k, pos_err, psel, hit, occ_dec):
            return finish(False)
        d, derr, cosn, dec = sample_lambert(u, first_n)
        pdf_w = max(cosn, 0.0) * INV_PI; pdf_k = derr / max(cosn, 1e-300)
        att = att * (rd1 / psel); att_k += 2.0
        cov["pt_lobe_lambert"] += 1; lobe = "lambert"
    else:
        if not add_nee(first_n, "P", rs1, e1, back, lp, ln, first_pos, att, att_k, pos_err, 1.0 - psel, hit, occ_dec):
            return finish(False)
        d, derr, unsafe, cos_r, dec = sample_phong(u, back, first_n, e1, 2.0)
        pdf_w = (e1 + 1.0) * 0.5 * max(cos_r, 0.0) ** e1 * INV_PI if unsafe > 0.0 else 0.0
        pdf_k = e1 * derr / max(cos_r, 1e-300)
        att = att * (rs1 * ((e1 + 2.0) / (e1 + 1.0) * max(unsafe, 0.0)) / (1.0 - psel)); att_k += 3.0 + (derr / unsafe if unsafe > 0.0 else 0.0)
        cov["pt_lobe_phong"] += 1; lobe = "phong"
    if not dec:
        return finish(False)
    prd = first_pos
    for i in range(max_bounces):
        done = i == max_bounces - 1
        tri, t, beta, gamma, dec = closest(G, prd, d, 1.0e-5); out.rays += 1
        if not dec:
            return finish(False)
        if tri < 0:
            cov["pt_miss"] += 1
            break
        gn = G.gn[tri]
        npos = prd + d * t
        front = float(gn @ d)
        if abs(front) < COS_MARGIN + (derr + pos_err / t) * ULP:
            return finish(False)
        if front > 0.0:                                                 # back face (:125-130)
            cov["pt_back_face"] += 1
            break
        # what the hit point is off by, in units of 2^-24: the origin's error and the direction's times the distance, along the surface
        # -- so divided by the cosine of incidence -- and the roundings of o + d t
        here_err = (pos_err + (derr + 2.0) * t) / abs(front) + POINT_ULPS * float(np.abs(npos).max())
        back_err = derr + (pos_err + here_err) / t                      # of the direction back along the ray, between two computed points
        if G.is_light[tri]:                                             # emitter reached by BRDF sampling (:133-148)
            cos_l = -front
            if G.lw != 0.0 and _near_cut(cos_l):
                return finish(False)
            if cos_l > CUT:
                bpa = pdf_w * cos_l / (t * t)                           # brdf_pdf_w * pdf_w2a(ffn, npos - prd)
                lpa = 1.0 / G.light_area
                w = bpa / (bpa + lpa) if bpa > 0.0 else 0.0
                fe = (G.lw + 2.0) * cos_l ** G.lw * INV_PI * 0.5        # PhongEvalF(gn, back, gn, lw): its cosine is cos_l
                dcos = (derr + here_err / t) / cos_l
                kappa = 6.0 + att_k + (pdf_k + dcos + 2.0 * here_err / t) * (lpa / (bpa + lpa)) + G.lw * dcos
                out.terms.append((att * w * fe * G.li, kappa))
            cov["pt_emitter_from_" + lobe] += 1
            break
        if done:                                                        # (:151)
            cov["pt_last_bounce"] += 1
            break
        k, lp, ln, dec = light_sample(G, u, cov)
        if not dec:
            return finish(False)
        hit, occ_dec = occluded(G, lp, npos - lp, 1.0e-5, float(np.float32(0.99999))); out.rays += 1
        kd, ks, ns, ktex, dec, textured = material_at(G, tri, beta, gamma, cov)
        if not dec:
            return finish(False)
        ml, mp = float(kd.max()), float(ks.max())
        if abs(ml + mp - BLACK) < BLACK_MARGIN:
            return finish(False)
        if ml + mp <= BLACK:                                            # (:172-173)
            cov["pt_black"] += 1
            break
        cov["pt_bounce:" + class_of(ks, ns, kd, textured)] += 1
        psel = ml / (mp + ml)
        choose = min(u(), CHOOSE_MAX)
        if abs(choose - psel) < SEL_ULPS * ULP * (1.0 + ktex):
            return finish(False)
        back = -d
        pos_err = here_err
        if choose < psel:
            if not add_nee(gn, "L", kd, ns, back, lp, ln, npos, att, att_k + 2.0 * ktex, pos_err, psel, hit, occ_dec, back_err):
                return finish(False)
            d, derr, cosn, dec = sample_lambert(u, gn)                  # the geometric normal (:197)
            pdf_w = max(cosn, 0.0) * INV_PI; pdf_k = derr / max(cosn, 1e-300)
            att = att * (kd / psel); att_k += 2.0 + 2.0 * ktex
            cov["pt_lobe_lambert"] += 1; lobe = "lambert"
        else:
            if not add_nee(gn, "P", ks, ns, back, lp, ln, npos, att, att_k + 2.0 * ktex + (ktex * ns if textured else 0.0), pos_err, 1.0 - psel, hit, occ_dec, back_err):
                return finish(False)
            d, derr, unsafe, cos_r, dec = sample_phong(u, back, gn, ns, back_err)
            pdf_w = (ns + 1.0) * 0.5 * max(cos_r, 0.0) ** ns * INV_PI if unsafe > 0.0 else 0.0
            pdf_k = ns * derr / max(cos_r, 1e-300)
            att = att * (ks * ((ns + 2.0) / (ns + 1.0) * max(unsafe, 0.0)) / (1.0 - psel)); att_k += 3.0 + 2.0 * ktex + (derr / unsafe if unsafe > 0.0 else 0.0)
            cov["pt_lobe_phong"] += 1; lobe = "phong"
        if not dec:
            return finish(False)
        russian = max(float(att.max()), RR_LT)                          # a MAX with 0.98 (pathtracing.cu:55)
        draw = u()
        m = RR_ULPS * ULP * (1.0 + att_k)                               # (att within m of 0.98, or the draw within m of att: undecided;
        if abs(float(att.max()) - RR_LT) < m * RR_LT or (russian > RR_LT and abs(draw - russian) < m * russian):    # the constant itself is exact)
            return finish(False)
        if draw >= russian:                                             # (:219-225)
            cov["pt_roulette_ended"] += 1
            break
        cov["pt_roulette_survived"] += 1
        prd = npos
        att = att / russian; att_k += 1.0
    return finish()


def path_image_f64(G, gbuf, names, cam, seed, max_bounces):
    """every stencilled pixel of the G-buffer.  Returns a namespace of [H, W] arrays: value [.., 3], A (sum of kappa_term |term|) [.., 3],
    S (sum of |term|) [.., 3], n (terms), decided, rays, stencil; and cov (Counter over decided pixels)"""
    pos, nrm, dif, phg = gbuf
    r = SimpleNamespace(value=np.zeros((H, W, 3)), A=np.zeros((H, W, 3)), S=np.zeros((H, W, 3)), n=np.zeros((H, W)), decided=np.zeros((H, W), bool),
                        rays=np.zeros((H, W), np.int64), stencil=pos[..., 3] != 0.0, cov=Counter())
    cam = np.asarray(cam, np.float32).astype(np.float64)
    for y in range(H):
        for x in range(W):
            if not r.stencil[y, x]:
                continue
            f = lambda a: a[y, x, :3].astype(np.float64)
            tags = names[y, x] if names is not None else ()
            cls = next((c for c in ("rsx_zero", "rsx_tiny", "pure_spec", "lambert_e_left") if c in tags), next((c for c in tags if c.startswith("e_")), None))
            o = path_pixel_f64(G, x, y, f(pos), f(nrm), f(dif), f(phg), float(phg[y, x, 3]), cam, seed, max_bounces, cls)
            r.decided[y, x] = o.decided; r.rays[y, x] = o.rays
            if o.decided:
                r.value[y, x] = o.value; r.n[y, x] = len(o.terms)
                for t, k in o.terms:
                    r.A[y, x] += k * np.abs(t); r.S[y, x] += np.abs(t)
                r.cov.update(o.cov)
    return r


def add_images(a, b):
    """two accumulated samples: the sum, its terms together"""
    return SimpleNamespace(value=a.value + b.value, A=a.A + b.A, S=a.S + b.S, n=a.n + b.n + 1, decided=a.decided & b.decided, rays=a.rays + b.rays,
                           stencil=a.stencil, cov=a.cov + b.cov)


def path_worst_ratio(got, ref):
    """the smallest K under which |x - f64| <= K 2^-24 sum kappa_term |term| + n_terms 2^-24 sum |term| + 1e-20 holds on the decided pixels,
    and the pixel it is met at.  A decided pixel without terms must be exactly 0: any other value gives inf."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref.value) - 1.0e-20 - ref.n[..., None] * ULP * ref.S
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / (ULP * ref.A), 0.0)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    ratio = np.where(ref.decided[..., None], ratio, 0.0)
    y, x, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[y, x, c]), (int(x), int(y), int(c))


# ------------------------------------------------------------------------------------------------------------------ the whole domain
class Domain:
    """the two scene variants, the receiver and the float64 answers of the path tracer, computed once per (exponent, seed, bounces)"""

    def __init__(self, oa):
        self.scenes = {e: patch_room(e) for e in LIGHT_EXPONENTS}
        self.geo = {e: Geometry(s) for e, s in self.scenes.items()}
        planes = oa.Scene(receiver_floor()).primary(W, H)                # the floor z = 0 under the whole frame, as the primary pass writes it
        self.gbuf, self.pixel_names = sd.make_receiver(planes[0], planes[1])
        self.gbuf[0][..., 2] = -Z0
        self.stencil = self.gbuf[0][..., 3] != 0.0
        self._pt = {}

    def pt_ref(self, exponent, seed, max_bounces):
        key = (exponent, seed, max_bounces)
        if key not in self._pt:
            self._pt[key] = path_image_f64(self.geo[exponent], self.gbuf, self.pixel_names, CAMERA, seed, max_bounces)
        return self._pt[key]


LT_ARMS = (tuple(f"lt_first:{c}" for c in CLASSES) + tuple(f"lt_bounce:{c}" for c in CLASSES)
           + ("lt_lobe_lambert", "lt_lobe_phong", "lt_roulette_survived", "lt_roulette_ended", "lt_end_miss", "lt_end_back_face", "lt_end_black", "lt_end_emitter",
              "light_triangle_0", "light_triangle_1", "light_triangle_2", "tex_u_below_0", "tex_u_above_1", "tex_v_below_0", "tex_v_above_1")
           + tuple(f"lt_ends_after_slot_{k}" for k in range(0, max(LT_P))))
PT_ARMS = (tuple(f"pt_first:{c}" for c in CLASSES if c != "textured") + tuple(f"pt_bounce:{c}" for c in CLASSES)
           + ("pt_lobe_lambert", "pt_lobe_phong", "pt_roulette_survived", "pt_roulette_ended", "pt_miss", "pt_back_face", "pt_black", "pt_emitter_from_lambert",
              "pt_emitter_from_phong", "nee_lit_lambert", "nee_lit_phong", "nee_occluded", "nee_unoccluded", "light_triangle_0", "light_triangle_1",
              "light_triangle_2", "tex_u_below_0", "tex_u_above_1", "tex_v_below_0", "tex_v_above_1"))


def check_arms(cov, arms, small_light=3):
    empty = [a for a in arms if cov[a] == 0]
    assert not empty, f"arms no decided sample visits: {empty}"
    assert cov["light_triangle_2"] >= small_light, cov["light_triangle_2"]
