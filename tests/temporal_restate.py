"""numpy fp32 restatements of the temporal accumulation (include/evplp.h evplp_denoise_temporal, evplp_project_points): every operation
rounded on its own, in the order of evplp_types.h project_point and kernels_temporal.hip.  Shared by tests/test_temporal_host.py (no GPU) and
tests/test_gpu_temporal.py."""
import math

import numpy as np

F = np.float32
Y = np.array([0.2126, 0.7152, 0.0722], F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def camera_basis(origin, lookat, up, fovy, aspect):
    """evplp_set_camera's basis (context.cpp camera_basis): dict of eye, s, u, f (float32 (3,)), tan_half, aspect"""
    o, l, upv = (np.asarray(v, F) for v in (origin, lookat, up))

    def norm(v):
        inv = F(1) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        return (v * inv).astype(F)

    def cross(a, b):
        return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)
    f = norm(l - o)
    s = norm(cross(f, upv))
    u = cross(s, f)
    return dict(eye=o, s=s, u=u, f=f, tan_half=F(math.tan(float(F(fovy) / F(2)))), aspect=F(aspect))


def project(cam, W, H, pts):
    """project_point for points (..., 3): (xyd (..., 3) float32, in front of the eye (...) bool)"""
    p = np.asarray(pts, F)
    d = p - cam["eye"]
    z = _dot(d, np.broadcast_to(cam["f"], d.shape))
    ok = z > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = _dot(d, np.broadcast_to(cam["s"], d.shape)); b = _dot(d, np.broadcast_to(cam["u"], d.shape))
        at = F(cam["aspect"] * cam["tan_half"])
        cx = (a / z) / at; cy = (b / z) / cam["tan_half"]
        x = ((cx + F(1)) * F(W)) / F(2) - F(0.5); y = ((cy + F(1)) * F(H)) / F(2) - F(0.5)
    out = np.stack([np.where(ok, x, F(0)), np.where(ok, y, F(0)), z], -1).astype(F)
    return out, ok


def primary_points(cam, W, H, xs, ys, t):
    """points at parameter t on the primary rays of primary_body.hpp (no jitter) through the centres of pixels (xs, ys)"""
    cx = (xs.astype(F) + F(0.5)) / F(W) * F(2) - F(1); cy = (ys.astype(F) + F(0.5)) / F(H) * F(2) - F(1)
    jx = cx * cam["aspect"] * cam["tan_half"]; jy = cy * cam["tan_half"]
    d = cam["s"] * jx[..., None] + cam["u"] * jy[..., None] + cam["f"]
    return (cam["eye"] + d * np.asarray(t, F)[..., None]).astype(F)


def pack(rgb, var, pos, nrm, dif, phg, light, image_rows):
    """denoise_prepare_kernel: (u (R, W, 4) = (u.rgb, s), filtered (R, W) bool, albedo (R, W, 3)) from resolve's composite, the variance,
    the guides and the light plane"""
    rgb, var = rgb.astype(F), var.astype(F)
    filt = (pos[..., 3] != 0) & (light[..., 0] == 0) & (light[..., 1] == 0) & (light[..., 2] == 0)
    filt[image_rows:] = False
    a = np.maximum(dif[..., :3] + phg[..., :3], F(1e-3))
    yy = Y * Y
    with np.errstate(over="ignore", invalid="ignore"):
        s = ((yy[0] * var[..., 0]) / (a[..., 0] * a[..., 0]) + (yy[1] * var[..., 1]) / (a[..., 1] * a[..., 1])) + (yy[2] * var[..., 2]) / (a[..., 2] * a[..., 2])
        uf = rgb / a
    filt &= np.isfinite(uf).all(-1) & np.isfinite(s)              # a pixel whose demodulated colour or s is not finite is not filtered
    u = np.where(filt[..., None], uf, rgb)
    return np.concatenate([u, np.where(filt, s, F(0))[..., None]], -1).astype(F), filt, a


def prev_pose(debug, prev_verts):
    """prev_pose_kernel's two expressions on the debug plane's (tri, b, g) and the previous vertices (ntri, 3, 3): (pos, nrm) (R, W, 4)"""
    tri = debug[..., 0].copy().view(np.int32)
    b, g = debug[..., 1], debug[..., 2]
    hit = tri >= 0
    v = prev_verts.astype(F)[np.where(hit, tri, 0)]
    p0, p1, p2 = v[..., 0, :], v[..., 1, :], v[..., 2, :]
    w0 = F(1) - b - g
    P = (p1 * b[..., None] + p2 * g[..., None]) + p0 * w0[..., None]
    e0, e1 = p1 - p0, p2 - p0
    c = np.stack([e0[..., 1] * e1[..., 2] - e0[..., 2] * e1[..., 1], e0[..., 2] * e1[..., 0] - e0[..., 0] * e1[..., 2],
                  e0[..., 0] * e1[..., 1] - e0[..., 1] * e1[..., 0]], -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1) / np.sqrt(_dot(c, c))
        N = c * inv[..., None]
    pos = np.concatenate([P, np.ones_like(b)[..., None]], -1); nrm = np.concatenate([N, np.zeros_like(b)[..., None]], -1)
    z = np.zeros_like(pos)
    return np.where(hit[..., None], pos, z).astype(F), np.where(hit[..., None], nrm, z).astype(F)


def accumulate(u, filt, pos, nrm, prev_pos, prev_nrm, hist, cam, prev_cam, W, H, sxr, normal_cos=0.9, max_history=16):
    """temporal_accumulate_kernel over a frame of (R, W) pixels.  u (R, W, 4) = (u.rgb, s); filt (R, W); pos, nrm (R, W, >= 3) the frame's
    position and normal; prev_pos / prev_nrm (R, W, 4) the previous-pose texels; hist = None (a first call) or the previous call's
    (h_u, h_pos, h_nrm).  Returns (u_out (R, W, 4), the new history (h_u, h_pos, h_nrm), dict of reprojected / taps / integral (R, W)
    and the four counts)."""
    R = u.shape[0]
    sxr, cosb, nmax = F(sxr), F(normal_cos), F(max_history)
    X = pos[..., :3].astype(F); n = nrm[..., :3].astype(F)
    sw = np.zeros((R, W), F); acc = np.zeros((R, W, 3), F); ss = np.zeros((R, W), F); nmin = np.full((R, W), F(3.0e38))
    taps = np.zeros((R, W), np.int32); integral = np.zeros((R, W), bool)
    if hist is not None:
        hu, hp, hn = hist
        P = prev_pos[..., :3].astype(F); N = prev_nrm[..., :3].astype(F)
        was, seen = project(prev_cam, W, H, P); is_, sees = project(cam, W, H, X)
        ys, xs = np.meshgrid(np.arange(R), np.arange(W), indexing="ij")
        with np.errstate(invalid="ignore", over="ignore"):
            fx = xs.astype(F) + (was[..., 0] - is_[..., 0]); fy = ys.astype(F) + (was[..., 1] - is_[..., 1])
            go = filt & (prev_pos[..., 3] != 0) & seen & sees & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
        fx = np.where(go, fx, F(0)); fy = np.where(go, fy, F(0))
        flx, fly = np.floor(fx), np.floor(fy)
        tx, ty = fx - flx, fy - fly
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        integral = go & (tx == 0) & (ty == 0)
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            ok = go & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            if k > 0:
                ok &= ~integral
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            hx, hnq, huq = hp[cy, cx], hn[cy, cx], hu[cy, cx]
            ok &= hx[..., 3] != 0
            Xq, nq = hx[..., :3], hnq[..., :3]
            with np.errstate(invalid="ignore", over="ignore"):
                d1 = np.abs(_dot(nq, P - Xq)); d2 = np.abs(_dot(N, Xq - P)); cs = _dot(N, nq)
                ok &= (d1 <= sxr) & (d2 <= sxr) & (cs >= cosb)
                w = ((tx if k & 1 else F(1) - tx) * (ty if k >> 1 else F(1) - ty)).astype(F)
                w = np.where(integral, F(1), w)
                sw = np.where(ok, sw + w, sw)
                acc = np.where(ok[..., None], acc + w[..., None] * huq[..., :3], acc)
                ss = np.where(ok, ss + (w * w) * huq[..., 3], ss)
            nmin = np.where(ok, np.minimum(nmin, hnq[..., 3]), nmin)
            taps += ok
    rep = filt & (sw > 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        length = np.minimum(nmin + F(1), nmax)
        al = F(1) / length; be = F(1) - al
        hs = ss / (sw * sw)
        rgb = be[..., None] * (acc / sw[..., None]) + al[..., None] * u[..., :3]
        s = (be * be) * hs + (al * al) * u[..., 3]
    out = np.where(rep[..., None], np.concatenate([rgb, s[..., None]], -1), u).astype(F)
    length = np.where(rep, length, np.where(filt, F(1), F(0))).astype(F)
    h_pos = np.concatenate([X, filt.astype(F)[..., None]], -1).astype(F)
    h_nrm = np.concatenate([n, length[..., None]], -1).astype(F)
    info = dict(reprojected=rep, taps=taps, integral=integral, filtered=int(filt.sum()), n_reprojected=int(rep.sum()),
                disoccluded=int((filt & ~rep).sum()) if hist is not None else 0, history_sum=int(length[filt].sum()))
    return out, (out.copy(), h_pos, h_nrm), info
