"""The probe gather (include/evplp.h "probe gather") restated in float64 numpy on the float32 inputs: the term of one (record, point) pair
with its conditioning, the order-2 real spherical-harmonic basis, and the irradiance of a coefficient set.  numpy only.

pair_f64 forms kappa, lam and decided the way shading_domain.vpl_pair_f64 does, with the receiver taken away:
  kappa   1 + 1 / cos2 (the VPL-side cosine -n2 . v12 is a difference of products) + e / d where the VPL's lobe is taken, and PER
          COEFFICIENT the conditioning of the basis function where it is itself a difference: Y6 = 0.315 (3 z^2 - 1) adds
          (3 z^2 + 1) / |3 z^2 - 1|, Y8 = 0.546 (x^2 - y^2) adds (x^2 + y^2) / |x^2 - y^2| -- the same rule (a difference has
          sum / |difference| times the rounding of its terms).  The other seven are products: nothing to add.
  lam     e |log2 d| of the lobe power the kernel takes as exp2(e log2 d)
  decided False where the cosine test or the lobe cut lies within shading_domain.COS_MARGIN
The kernel's max(dist2, min_distance^2) is continuous: it needs no margin.

A pair whose float32 dist2 is not a normal finite number casts no ray and adds no term (include/evplp.h): walked_f32 decides it on the
kernel's own bits, as facing_f32 decides the cosine test, and pair_f64 takes that decision over -- the rule is stated on those bits, so
there is no float64 version of it and nothing undecided about it.
"""
import math

import numpy as np

import shading_domain as sd

Y_CONST = (0.28209479, 0.48860251, 1.09254843, 0.31539157, 0.54627422)      # the header's constants, as written there
BAND = np.array([math.pi] + [2.0 * math.pi / 3.0] * 3 + [math.pi / 4.0] * 5)


def _c(k):
    return float(np.float32(Y_CONST[k]))


def basis_f64(w):
    """Y_0 .. Y_8 of directions w [..., 3] (taken as given), float64 [..., 9], with the header's constants rounded to float32"""
    w = np.asarray(w, np.float64)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    return np.stack([np.full_like(x, _c(0)), _c(1) * y, _c(1) * z, _c(1) * x, _c(2) * x * y, _c(2) * y * z, _c(3) * (3.0 * z * z - 1.0),
                     _c(2) * x * z, _c(4) * (x * x - y * y)], -1)


def basis_abs_f64(w):
    """the sum of the magnitudes of the terms each Y_i is formed from (what a float32 evaluation's rounding is relative to)"""
    w = np.asarray(w, np.float64)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    b = np.abs(basis_f64(w))
    b[..., 6] = _c(3) * (3.0 * z * z + 1.0)
    b[..., 8] = _c(4) * (x * x + y * y)
    return b


def basis_exact(w):
    """the basis with the exact constants sqrt(1 / 4 pi) ...: what the header's eight digits stand for"""
    w = np.asarray(w, np.float64)
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    k0, k1, k2, k3, k4 = (0.5 * math.sqrt(1.0 / math.pi), math.sqrt(3.0 / (4.0 * math.pi)), 0.5 * math.sqrt(15.0 / math.pi),
                          0.25 * math.sqrt(5.0 / math.pi), 0.25 * math.sqrt(15.0 / math.pi))
    return np.stack([np.full_like(x, k0), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * (3.0 * z * z - 1.0), k2 * x * z, k4 * (x * x - y * y)], -1)


def irradiance_f64(c, normal):
    """the clamped-cosine convolution of coefficients c [..., 9, 3] at unit normals [..., 3]: sum_i A_l(i) Y_i(n) c_i, float64 [..., 3]"""
    y = basis_f64(normal)
    return ((BAND * y)[..., None] * np.asarray(c, np.float64)).sum(-2)


def irradiance_abs_f64(c, normal):
    y = basis_abs_f64(normal)
    return ((BAND * y)[..., None] * np.abs(np.asarray(c, np.float64))).sum(-2)


def facing_f32(record, x):
    """the kernel's cosine test on its own bits: c2 = -((n.x v.x + n.y v.y) + n.z v.z) > 0 with every float32 operation rounded on its
    own; and v12 in float32 (the shadow ray's direction is -v12)"""
    F = np.float32
    x = np.asarray(x, F).reshape(-1, 3)
    v12 = (np.asarray(record["pos"], F)[None, :] - x).astype(F)
    n = np.asarray(record["normal"], F)
    p = (n[None, :] * v12).astype(F)
    d = ((p[:, 0] + p[:, 1]).astype(F) + p[:, 2]).astype(F)
    return (-d) > 0, v12


def walked_f32(record, x):
    """the kernel's test of dist2 = (v.x v.x + v.y v.y) + v.z v.z, every float32 operation rounded on its own (subnormals kept): True where
    it is a normal finite number, 2^-126 <= dist2 <= FLT_MAX.  Only such a pair casts a shadow ray and adds a term."""
    F = np.float32
    x = np.asarray(x, F).reshape(-1, 3)
    v12 = (np.asarray(record["pos"], F)[None, :] - x).astype(F)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        p = (v12 * v12).astype(F)
        d2 = ((p[:, 0] + p[:, 1]).astype(F) + p[:, 2]).astype(F)
    return (d2 >= F(2.0 ** -126)) & (d2 <= np.finfo(F).max)


def pair_f64(record, x, min_distance):
    """one record against points x [n, 3] (finite), visibility 1.  Returns term [n, 9, 3] (E Y_i, NOT divided by the path count),
    kappa [n, 9, 1], lam [n, 9], decided [n], facing [n] (the pair passes the cosine test and walked_f32: it casts a shadow ray)."""
    v = sd._rec64(record)
    x = np.asarray(x, np.float32).astype(np.float64).reshape(-1, 3)
    md2 = float(np.float32(min_distance)) ** 2
    v12 = v.pos - x
    c2u = -sd._dot(v12, v.n)
    walked = walked_f32(record, x)
    facing = (c2u > 0.0) & walked
    dist2 = sd._dot(v12, v12)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.sqrt(dist2)
        w = np.where(dist[:, None] > 0.0, v12 / dist[:, None], 0.0)
        cos2 = np.where(dist > 0.0, c2u / dist, 0.0)
    decided = ~(np.abs(cos2) < sd.COS_MARGIN)
    kappa = 1.0 + 1.0 / np.maximum(cos2, 1e-300)
    lam = np.zeros_like(dist)
    ph2 = np.zeros_like(dist)
    if bool(np.any(v.rs != 0.0)):                                               # PhongEvalF(-w, fluxDir, n2, e2), rtmaterial.cuh:112-118
        d2 = sd._dot(-w, 2.0 * v.n * np.dot(v.n, v.fdir) - v.fdir)
        on2 = d2 > sd.CUT_CUDA
        ph2 = np.where(on2, (v.e + 2.0) * sd._pow(d2, v.e) * sd.INV_PI * 0.5, 0.0)
        decided &= ~sd._near_cut(d2, sd.CUT_CUDA)
        kappa = kappa + np.where(on2, v.e / np.maximum(d2, sd.CUT_CUDA), 0.0)
        lam = lam + np.where(on2, v.e * np.abs(np.log2(np.maximum(d2, sd.CUT_CUDA))), 0.0)
    brdf2 = v.rd * sd.INV_PI + v.rs * ph2[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(facing, cos2 / np.maximum(dist2, md2), 0.0)
    E = v.flux * brdf2 * g[:, None]                                             # [n, 3]
    Y, Yabs = basis_f64(w), basis_abs_f64(w)
    term = Y[:, :, None] * E[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        ycond = np.where(np.abs(Y) > 0.0, Yabs / np.abs(Y), 1.0) - 1.0          # 0 for the products
    kap = (np.where(facing, kappa, 1.0)[:, None] + np.minimum(ycond, 1e30))[:, :, None]
    lam9 = np.repeat(np.where(facing, lam, 0.0)[:, None], 9, axis=1)
    term = np.where(facing[:, None, None], term, 0.0)
    return term, kap, lam9, decided | ~walked, facing                           # (a skipped pair is exactly 0 whatever its cosines)
