"""Lightmap baking (include/evplp.h "lightmap baking") restated in numpy: the surface point of a hit in float32 with one rounding per
operation (primary_body.hpp's hit point, the flat winding normal with the oracle's roundings, material_at and tex2d of device_common.hpp),
the atlas rasteriser in int64, and the resolve and the gutter of the bake.  numpy only; nothing here calls the library.

Every float32 expression below is written so that numpy rounds after each operation: operands are float32 arrays, never Python floats
(those would promote to float64)."""
import numpy as np

F = np.float32
SUB = 256
MAX_SNAP = 1 << 22


# ---------------------------------------------------------------------------------------------------------------- points
def _wrap(i, n):
    return np.mod(i, n)            # (numpy's mod takes the divisor's sign: wrapi)


def tex2d(tex, u, v):
    """device_common.hpp tex2d on a texture [h, w, 4] float32 at float32 coordinate arrays: [n, 4]"""
    h, w = tex.shape[:2]
    if w == 1 and h == 1:
        return np.broadcast_to(tex[0, 0], (len(u), 4)).astype(F)
    xb = u * F(w) - F(0.5); yb = v * F(h) - F(0.5)
    xf = np.floor(xb); yf = np.floor(yb)
    a = (xb - xf).astype(F); b = (yb - yf).astype(F)
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1, y0, y1 = _wrap(xi, w), _wrap(xi + 1, w), _wrap(yi, h), _wrap(yi + 1, h)
    p00, p10, p01, p11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    one = F(1.0)
    w00 = ((one - a) * (one - b))[:, None]; w10 = (a * (one - b))[:, None]; w01 = ((one - a) * b)[:, None]; w11 = (a * b)[:, None]
    return (((w00 * p00 + w10 * p10) + w01 * p01) + w11 * p11).astype(F)


def dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def surface_points(sd, hits, flags=0, eyes=None, point_dtype=None):
    """evplp_surface_points over a scenes.SceneData: hits a HIT_DTYPE-like structured array (beta, gamma, triangle); returns float32 [n, 16]"""
    V, U, M = sd.triangle_soup()
    n = len(hits)
    out = np.zeros((n, 16), F)
    tri = hits["triangle"].astype(np.int64)
    b, g = hits["beta"].astype(F), hits["gamma"].astype(F)
    with np.errstate(all="ignore"):
        ok = (tri >= 0) & (tri < len(V)) & np.isfinite(b) & np.isfinite(g)
        t = np.where(ok, tri, 0)
        p0, p1, p2 = V[t, 0:3], V[t, 3:6], V[t, 6:9]
        w0 = (F(1.0) - b) - g
        P = ((p1 * b[:, None] + p2 * g[:, None]) + p0 * w0[:, None]).astype(F)
        e1, e2 = p1 - p0, p2 - p0
        cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]; cy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]; cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        c = np.stack([cx, cy, cz], -1).astype(F)
        inv = F(1.0) / np.sqrt(dot32(c, c)).astype(F)
        N = (c * inv[:, None]).astype(F)
        ok &= np.isfinite(N).all(-1)
        kd = np.ones((n, 3), F); ks = np.zeros((n, 3), F); ns = np.zeros(n, F)
        if not (flags & 1):
            for mi, m in enumerate(sd.materials):
                sel = ok & (M[t] == mi)
                if not sel.any():
                    continue
                kd[sel] = np.asarray(m["kd"], F); ks[sel] = np.asarray(m["ks"], F); ns[sel] = F(m["ns"])
                if m["tex_kd"] >= 0 or m["tex_ks"] >= 0 or m["tex_ns"] >= 0:
                    uv = U[t[sel]]; bb, gg = b[sel], g[sel]
                    ww = (F(1.0) - bb) - gg
                    u = (uv[:, 2] * bb + uv[:, 4] * gg) + uv[:, 0] * ww
                    v = (uv[:, 3] * bb + uv[:, 5] * gg) + uv[:, 1] * ww
                    if m["tex_kd"] >= 0:
                        kd[sel] = tex2d(sd.textures[m["tex_kd"]], u, v)[:, :3]
                    if m["tex_ks"] >= 0:
                        ks[sel] = tex2d(sd.textures[m["tex_ks"]], u, v)[:, :3]
                    if m["tex_ns"] >= 0:
                        ns[sel] = tex2d(sd.textures[m["tex_ns"]], u, v)[:, 0]
        if flags & 2:
            flip = dot32(N, np.asarray(eyes, F) - P) < 0
            N = np.where(flip[:, None], -N, N)
    out[:, 0:3] = P; out[:, 3] = 1.0; out[:, 4:7] = N; out[:, 8:11] = kd; out[:, 12:15] = ks; out[:, 15] = ns
    out[~ok] = 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------- the rasteriser
def snap(u, size):
    """rint(fl(fl(u * size) * 256)) as int64, and whether it is representable (|.| <= 2^22)"""
    with np.errstate(all="ignore"):
        r = np.rint((np.asarray(u, F) * F(size)).astype(F) * F(256.0)).astype(F)
        ok = np.abs(r) <= F(MAX_SNAP)            # (False for a NaN)
    return np.where(ok, r, 0).astype(np.int64), ok


def edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def owns(dx, dy):
    return (dy > 0) | ((dy == 0) & (dx < 0))


def sample_positions(size, S):
    """the sample coordinates of one axis, [size * S]: texel x, sample i at index x * S + i"""
    x = np.arange(size, dtype=np.int64)[:, None]; i = np.arange(S, dtype=np.int64)[None, :]
    return (SUB * x + (2 * i + 1) * (128 // S)).reshape(-1)


def cover_one(uv6, width, height, px, py):
    """one triangle (6 floats) against sample coordinate arrays px, py (int64, broadcastable): (inside, beta, gamma)"""
    uv6 = np.asarray(uv6, F)
    X, okx = snap(uv6[0::2], width); Y, oky = snap(uv6[1::2], height)
    px, py = np.broadcast_arrays(np.asarray(px, np.int64), np.asarray(py, np.int64))
    none = np.zeros(px.shape, bool), np.zeros(px.shape, F), np.zeros(px.shape, F)
    if not (okx.all() and oky.all()):
        return none
    a2 = int(edge(X[0], Y[0], X[1], Y[1], X[2], Y[2]))
    if a2 == 0:
        return none
    mirrored = a2 < 0
    if mirrored:
        X = X[[0, 2, 1]]; Y = Y[[0, 2, 1]]; a2 = -a2
    inside = np.ones(px.shape, bool)
    E = []
    for k in range(3):
        a, b = k, (k + 1) % 3
        e = edge(X[a], Y[a], X[b], Y[b], px, py)
        inside &= (e > 0) | ((e == 0) & bool(owns(X[b] - X[a], Y[b] - Y[a])))
        E.append(e)
    beta = (E[2].astype(np.float64) / np.float64(a2)).astype(F); gamma = (E[0].astype(np.float64) / np.float64(a2)).astype(F)
    if mirrored:
        beta, gamma = gamma, beta
    return inside, np.where(inside, beta, F(0)), np.where(inside, gamma, F(0))


def rasterise(uvs, first, width, height, S, hit_dtype):
    """evplp_lightmap_samples: uvs [k, 6] of the scene triangles first .. first + k - 1; returns hit_dtype [height, width, S, S]"""
    px = sample_positions(width, S)[None, :]; py = sample_positions(height, S)[:, None]
    tri = np.full((height * S, width * S), -1, np.int32)
    beta = np.zeros(tri.shape, F); gamma = np.zeros(tri.shape, F)
    for k in range(len(uvs) - 1, -1, -1):              # descending: the lowest index is written last and wins
        inside, b, g = cover_one(uvs[k], width, height, px, py)
        if inside.any():
            tri[inside] = first + k; beta[inside] = b[inside]; gamma[inside] = g[inside]
    out = np.zeros((height, width, S, S), hit_dtype)
    for name, a in (("triangle", tri), ("beta", beta), ("gamma", gamma)):
        out[name] = a.reshape(height, S, width, S).transpose(0, 2, 1, 3)      # [y, j, x, i] -> [y, x, j, i]
    return out


# ---------------------------------------------------------------------------------------------------------------- the bake
def resolve(valid, vpl, pm, photons, texel_dtype):
    """the samples of an atlas ([H, W, S, S] valid bool, vpl / pm [H, W, S, S, 3], photons [H, W, S, S]) to texels [H, W]: the float32 sums
    in ascending (j, i), divided by the count"""
    H, W, S = valid.shape[:3]
    out = np.zeros((H, W), texel_dtype)
    sv = np.zeros((H, W, 3), F); sp = np.zeros((H, W, 3), F); sn = np.zeros((H, W), F); cnt = np.zeros((H, W), F)
    for j in range(S):
        for i in range(S):
            m = valid[:, :, j, i]
            sv = np.where(m[..., None], sv + vpl[:, :, j, i].astype(F), sv); sp = np.where(m[..., None], sp + pm[:, :, j, i].astype(F), sp)
            sn = np.where(m, sn + photons[:, :, j, i].astype(F), sn); cnt = cnt + m.astype(F)
    some = cnt > 0
    d = np.where(some, cnt, F(1))
    out["vpl"] = np.where(some[..., None], sv / d[..., None], F(0)); out["pm"] = np.where(some[..., None], sp / d[..., None], F(0))
    out["photons"] = np.where(some, sn / d, F(0)); out["coverage"] = np.where(some, cnt / F(S * S), F(0))
    return out


NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))


def gutter(texels, passes):
    """the bake's dilation: texels [H, W] of the texel dtype, `passes` passes, each reading the state before it"""
    cur = texels.copy()
    H, W = cur.shape
    for d in range(1, passes + 1):
        flat = cur.view(F).reshape(H, W, 8)
        s = np.zeros((H, W, 8), F); n = np.zeros((H, W), F)
        for dx, dy in NEIGHBOURS:
            sh = np.zeros((H, W, 8), F)
            ys, yd = (slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0)))
            xs, xd = (slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0)))
            sh[yd, xd] = flat[ys, xs]
            m = sh[..., 3] != 0
            s = np.where(m[..., None], s + sh, s); n = n + m.astype(F)
        take = (flat[..., 3] == 0) & (n > 0)
        nd = np.where(take, n, F(1))
        new = (s / nd[..., None]).astype(F)
        new[..., 3] = -F(d)
        nxt = np.where(take[..., None], new, flat)
        cur = np.ascontiguousarray(nxt).view(texels.dtype).reshape(H, W)
    return cur
