"""Hostile planes for the a-trous denoiser (evplp_denoise, kernels_denoise.hip) and its two references (numpy only, no GPU).

The other denoiser tests see natural renders of the box room at the default parameters.  Here the caller chooses every plane: the four
G-buffer planes, the light plane and the accumulators are uploaded, the noise tracker is folded over uploaded sums (the per-fold
increments set each pixel's variance), and evplp_denoise runs on that.  drive() does it on a context; host_inputs() builds the composite
and the variance the library would hand out from the same planes in numpy (resolve_kernel's expression, test_gpu_noise.numpy_variance), so
that tests/test_denoise_hostile_host.py can prove what the cases are and measure the bars without a device.

Planes.  A frame is W x H image pixels in `rows` = 8 ceil(H / 8) plane rows (a whole context's local_rows), y = 0 at the bottom.  EVERY
ROW PAST H holds position.w = 1, a zero light plane and 1e30 (even columns) or NaN (odd columns) in everything else, accumulators
included: by its planes such a pixel is a surface and no emitter, and only the `y < H` test of denoise_prepare_kernel keeps it out.
(In the even columns u = 2e30 / 4 / 2e30 and s = 0 are finite; as a tap such a pixel has weight exp(-huge) * Inf = NaN.)
The image rows are a tilted plane through a camera-less world (no ray is traced: the scene of scene() is there for its bounding radius
alone, RADIUS = 1.5 exactly), 0.02 apart per pixel, with a bump of 0.004 along the normal (the position term |n . d| / (0.01 R) between
0 and about 0.5 inside the footprint), a depth step of 0.05 at x >= 0.6 W (3.3 in that term: a weight of a few per cent, not zero) and a
normal crease at y >= H / 2 (n . n' = 0.989, to the 128th: 0.24).  Colours are non-negative, so every sum of the filter is a sum of
non-negative terms and a relative bar means what it says.

Families (make_case):
  smooth         an albedo gradient, a smooth signal, FOLDS = 4 increments of signal * (1 + 0.3 N(0, 1)) clipped at 0
  holes          smooth with position.w = 0 on about half the pixels (their accumulators hold 50: a tap that is taken shows), the light
                 plane non-zero in R only, G only, B only on three disjoint tenths, one filtered pixel whose eight neighbours are all
                 unfiltered (three of them the three kinds of emitter), and filtered pixels in the four corners
  zero_variance  identical dyadic increments in every fold (Q - S^2 / K = 0 exactly), one albedo, a two-valued image in blocks of 3 x 2
  dark           diffuse + phong of exactly 0, 5e-4 and 1e-3 (= 5e-4 + 5e-4 in fp32) by column, every fourth column per-channel albedos
                 (1e-3, 0.03, 1) rotated by row
  normals        a zero normal on about 5 % of the pixels (sum w = 0: the pixel is kept) and a band of columns whose normals alternate
                 between n and -n
  bright         the signal times 10^(-6 .. 6) along x (a factor 2.2 per pixel at W = 37), noise in proportion
  nonfinite      smooth with single pixels, six or more apart, of four kinds: an accumulator of +Inf, one of NaN, sums of 1e20 whose
                 increments (1e20, 3e20, ...) give a variance beyond fp32 (Q is fp64: the accumulators are finite), and a finite composite
                 of 2^120 = 1.3e36 on an albedo at the floor (u = c / 1e-3 overflows; the composite is finite and the variance 0).
                 make_case(..., masked=True) is the same frame with position.w = 0 on those pixels.

References.  restate() is the fp32 restatement in the kernels' operation order that tests/test_gpu_denoise.py has always used (it lives
here now and that file imports it back); with fn64=True its exp, pow and sqrt are evaluated in float64 and rounded to fp32, which is how
the host test measures how far those functions' last bits can carry.  statement64() is the formula of include/evplp.h in float64, written
from the header's text alone: it shares no line with restate() (other than the luminance weights), pads and slices where restate() shifts
and masks, and takes every sum in float64.  Where sum w = 0 the header's quotient has no value; the pixel is kept, as the kernel's comment
says."""
from types import SimpleNamespace

import numpy as np

import scenes
from test_gpu_noise import numpy_variance

f32, f64 = np.float32, np.float64
Y = np.array([0.2126, 0.7152, 0.0722], np.float32)
B5 = [1.0 / 16.0, 0.25, 0.375, 0.25, 1.0 / 16.0]
B3 = [0.25, 0.5, 0.25]

FAMILIES = ("smooth", "holes", "zero_variance", "dark", "normals", "bright", "nonfinite")
FRAMES = ((37, 21), (259, 13), (5, 3))
CASES = [(fam, 37, 21) for fam in FAMILIES] + [(fam, w, h) for w, h in FRAMES[1:] for fam in ("smooth", "holes")]
F64_FAMILIES = ("smooth", "holes", "dark", "bright")      # zero_variance is excluded (see tests/test_denoise_hostile_host.py)
FOLDS = 4
RADIUS = 1.5                                              # scene()'s bounding-sphere radius: half the diagonal of a 2 x 2 x 1 box
KINDS = ("inf", "nan", "variance", "overflow")


def case_id(case):
    return "%s-%dx%d" % tuple(case)


def plane_rows(H):
    return (H + 7) // 8 * 8


def scene():
    """any small scene: evplp_denoise wants a built tree for its bounding radius and nothing else"""
    s = scenes.SceneData()
    grey = s.add_material((0.5, 0.5, 0.5))
    s.add_box((0.0, 0.0, 0.0), (2.0, 2.0, 1.0), grey, outward=False)
    s.light_mesh = s.add_quad([0.75, 0.75, 0.95], [0.0, 0.5, 0.0], [0.5, 0.0, 0.0], s.add_material((0, 0, 0)))
    s.cam_origin = [1.0, 0.2, 0.5]; s.cam_lookat = [1.0, 1.8, 0.5]
    s.triangle_soup()
    return s


# ---- the planes
def _unit(v):
    v = np.asarray(v, f64)
    return v / np.linalg.norm(v)


def _surface(W, H):
    """position, normal (H, W, 3) in float64 and the pixel indices"""
    jj, ii = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    n0 = _unit([0.3, -0.2, 1.0])
    e1 = _unit(np.cross([0.0, 1.0, 0.0], n0)); e2 = np.cross(n0, e1)
    along = 0.004 * np.sin(0.7 * ii) * np.cos(0.5 * jj) + np.where(ii >= 0.6 * W, 0.05, 0.0)
    P = np.array([0.4, 0.3, 0.2]) + 0.02 * ii[..., None] * e1 + 0.02 * jj[..., None] * e2 + along[..., None] * n0
    n1 = _unit(n0 + 0.15 * e2)
    N = np.where((jj >= H / 2)[..., None], n1, n0)
    return P, N, ii, jj, n0


def _signal(ii, jj):
    base = 1.0 + 0.5 * np.sin(0.3 * ii) + 0.3 * np.cos(0.4 * jj)
    return base[..., None] * np.array([1.0, 0.8, 0.6])


def _seed(family, W, H):
    return [FAMILIES.index(family), W, H, 20261021]


def make_case(family, W, H, masked=False):
    """the planes of one case: pos, nrm, dif, phg, light (rows, W, 4) fp32, sums = the FOLDS + 1 states of EVPLP_BUF_VPL_ACCUM (tracking starts
    at sums[0], one fold after each later one), photon = EVPLP_BUF_PHOTON_ACCUM (zero in the image), and what the family marks"""
    assert family in FAMILIES
    rng = np.random.default_rng(_seed(family, W, H))
    rows = plane_rows(H)
    P, N, ii, jj, n0 = _surface(W, H)
    xi, yi = ii.astype(np.int64), jj.astype(np.int64)
    dif = np.stack([0.2 + 0.6 * ii / W, 0.7 - 0.5 * jj / H, 0.3 + 0.4 * (ii + jj) / (W + H)], -1)
    phg = np.full((H, W, 3), 0.05)
    signal = _signal(ii, jj)
    noise = [1.0 + 0.3 * rng.standard_normal((H, W, 3)) for _ in range(FOLDS)]
    surface = np.ones((H, W), bool)
    light = np.zeros((H, W, 3))
    marks = {}
    exact = None                                            # increments given outright (H, W, 3) per fold, not albedo * signal * noise

    if family == "holes":
        surface = rng.random((H, W)) >= 0.5
        t = rng.random((H, W))
        cy, cx = H // 2, W // 2
        ring = [(cy + dy, cx + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
        for y, x in ring:
            surface[y, x] = False; t[y, x] = 1.0
        surface[cy, cx] = True; t[cy, cx] = 1.0
        kinds = [(0.8, 0.0, 0.0), (0.0, 0.7, 0.0), (0.0, 0.0, 0.9)]
        for k, col in enumerate(kinds):
            light[(t >= 0.1 * k) & (t < 0.1 * (k + 1))] = col
            y, x = ring[3 * k]
            light[y, x] = col; surface[y, x] = True          # an emitter pixel ON a surface: the light plane alone unfilters it
        for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
            surface[y, x] = True; light[y, x] = 0.0
        marks.update(isolated=(cy, cx), corners=((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)),
                     emitters=[(light[..., k] != 0) & (np.delete(light, k, -1) == 0).all(-1) for k in range(3)])
    elif family == "zero_variance":
        dif = np.broadcast_to(np.array([0.5, 0.375, 0.25]), (H, W, 3)).copy(); phg = np.zeros((H, W, 3))
        two = ((xi // 3 + yi // 2) % 2).astype(bool)
        exact = [np.where(two[..., None], np.array([0.75, 0.25, 0.5]), np.array([0.25, 0.5, 0.125]))] * FOLDS
        marks.update(two=two)
    elif family == "dark":
        col = xi % 4
        half = np.float64(f32(5e-4))
        dif = np.where((col == 0)[..., None], 0.0, half) * np.ones(3)
        phg = np.where((col == 2)[..., None], half, 0.0) * np.ones(3)
        span = np.array([1e-3, 0.03, 1.0])
        per_channel = np.stack([span[(np.arange(3) + r) % 3] for r in range(3)])[yi % 3]
        dif = np.where((col == 3)[..., None], per_channel, dif)
    elif family == "normals":
        zero = rng.random((H, W)) < 0.05
        zero[H // 3, W // 3] = True
        band = (xi >= W // 4) & (xi < W // 4 + 6)
        N = np.where((band & ((xi + yi) % 2 == 1))[..., None], -N, N)
        N = np.where(zero[..., None], 0.0, N)
        marks.update(zero_normal=zero, band=band)
    elif family == "bright":
        signal = signal * (10.0 ** (-6.0 + 12.0 * ii / max(W - 1, 1)))[..., None]

    albedo = np.maximum(dif.astype(f32) + phg.astype(f32), f32(1e-3)).astype(f64)
    incs = exact if exact is not None else [np.maximum(albedo * signal * nz, 0.0) for nz in noise]
    incs = [np.where(surface[..., None], d, 12.5) for d in incs]        # pixels that are no surface: 50 after four folds

    if family == "nonfinite":
        spots = [(y, x) for y in range(2, H - 2, 6) for x in range(2, W - 2, 6)]
        assert len(spots) >= 2 * len(KINDS), (W, H)
        picked = [spots[i] for i in rng.permutation(len(spots))[:2 * len(KINDS)]]
        kinds = {k: picked[2 * i:2 * i + 2] for i, k in enumerate(KINDS)}
        for y, x in kinds["overflow"]:
            dif[y, x] = 0.0; phg[y, x] = 0.0
        marks.update(kinds=kinds, bad=picked)
        if masked:
            for y, x in picked:
                surface[y, x] = False

    def plane(a, w=0.0):
        out = np.empty((rows, W, 4), f32)
        out[:H, :, :3] = a.astype(f32); out[:H, :, 3] = w
        out[H:, 0::2] = f32(1e30); out[H:, 1::2] = f32(np.nan)
        return out

    pos = plane(np.where(surface[..., None], P, 0.0), surface.astype(f32))
    pos[H:, :, 3] = 1.0
    light4 = plane(light); light4[H:] = 0.0
    sums = [np.zeros((rows, W, 4), f32)]
    for j, d in enumerate(incs):
        nxt = sums[-1].copy()
        nxt[:H, :, :3] = nxt[:H, :, :3] + d.astype(f32)
        sums.append(nxt)
    if family == "nonfinite":
        for n, (y, x) in enumerate(marks["kinds"]["inf"]):
            for j in range(2, FOLDS + 1):
                sums[j][y, x, n] = np.inf
        for n, (y, x) in enumerate(marks["kinds"]["nan"]):
            for j in range(1 + n, FOLDS + 1):
                sums[j][y, x, 1 + n] = np.nan
        for y, x in marks["kinds"]["variance"]:
            for j in range(1, FOLDS + 1):
                sums[j][y, x, :3] = sums[j - 1][y, x, :3] + f32(1e20 if j % 2 else 3e20)
        for y, x in marks["kinds"]["overflow"]:
            for j in range(1, FOLDS + 1):
                sums[j][y, x, :3] = f32(j) * f32(2.0 ** 120)                # (a power of two: the increments are identical, the variance is 0)
    for s in sums:                                          # (the same 1e30 in every state: a variance of 0 and u = 1 / 4, finite -- by the
        s[H:, 0::2] = f32(1e30); s[H:, 1::2] = f32(np.nan)  # rule for non-finite pixels alone such a pixel would still be filtered)
    photon = np.zeros((rows, W, 4), f32)
    photon[H:, 0::2] = f32(1e30); photon[H:, 1::2] = f32(np.nan)
    return SimpleNamespace(family=family, W=W, H=H, rows=rows, folds=FOLDS, scale=1.0 / FOLDS, pos=pos, nrm=plane(N), dif=plane(dif), phg=plane(phg),
                           light=light4, sums=sums, photon=photon, marks=marks, masked=masked)


def guides(case):
    return case.pos, case.nrm, case.dif, case.phg


def host_inputs(case, scale=None, light_scale=1.0, mask_emitter=False):
    """(rgb, var) (rows, W, 3) fp32 as evplp_resolve(scale, scale, light_scale, mask_emitter) and evplp_noise_variance(scale) give them
    for the case's planes: resolve_kernel's expression and the tracker's formula, in numpy"""
    scale = case.scale if scale is None else scale
    with np.errstate(over="ignore", invalid="ignore"):
        var = numpy_variance([(s[..., :3] + case.photon[..., :3]).astype(f32) for s in case.sums], (1,) * case.folds, scale).astype(f32)
        vs, ls = f32(scale), f32(light_scale)
        l = case.light[..., :3]
        step = np.where(f32(0) < l[..., :1] * ls, f32(0), f32(1)) if mask_emitter else f32(1)
        rgb = (step * (case.sums[-1][..., :3] * vs + case.photon[..., :3] * vs) + l * ls).astype(f32)
    return rgb, var


def drive(evplp, case, calls=((None, 1.0, False, {}),)):
    """evplp_denoise on the case's planes.  calls: (scale or None = 1 / folds, light_scale, mask_emitter, denoise keywords); per call a dict of
    den, den2 (a second call), rgb = resolve, var = noise_variance and the scale; the planes as downloaded, and the radius, under "planes"."""
    out = []
    with evplp.Context(case.W, case.H, 1, 1, 1) as c:
        scene().upload(c)
        radius = c.scene_metrics()[0]
        assert c.local_rows == case.rows and radius == RADIUS, (c.local_rows, radius)
        for b, p in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG, evplp.BUF_LIGHT),
                        guides(case) + (case.light,)):
            c.upload(b, p)
        c.upload(evplp.BUF_VPL_ACCUM, case.sums[0]); c.upload(evplp.BUF_PHOTON_ACCUM, case.photon)
        c.noise_track(True)
        for s in case.sums[1:]:
            c.upload(evplp.BUF_VPL_ACCUM, s)
            c.noise_fold(1)
        planes = [c.download(b) for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG, evplp.BUF_LIGHT)]
        for scale, ls, me, kw in calls:
            s = case.scale if scale is None else scale
            out.append(dict(scale=s, den=c.denoise(s, ls, me, **kw), rgb=c.resolve(s, s, ls, mask_emitter=me), var=c.noise_variance(s),
                            den2=c.denoise(s, ls, me, **kw), planes=planes, radius=radius))
    return out


# ---- the fp32 restatement
def _shift(a, dy, dx):
    """out[y, x] = a[y + dy, x + dx] inside the frame (zeros outside) and the in-frame mask"""
    rows, cols = a.shape[:2]
    out = np.zeros_like(a); ok = np.zeros((rows, cols), bool)
    ys, ye = max(0, -dy), min(rows, rows - dy); xs, xe = max(0, -dx), min(cols, cols - dx)
    if ys < ye and xs < xe:
        out[ys:ye, xs:xe] = a[ys + dy:ye + dy, xs + dx:xe + dx]; ok[ys:ye, xs:xe] = True
    return out, ok


def _in64(fn):
    return lambda *a: fn(*[np.asarray(x, f64) for x in a]).astype(f32)


def restate(rgb, var, pos, nrm, dif, phg, light, radius, image_rows, levels=5, sigma_l=4.0, sigma_n=128.0, sigma_x=0.01, fn64=False, kept=None):
    """include/evplp.h evplp_denoise in numpy, fp32 in the kernels' operation order; inputs in resolve's layout (rows from the bottom).
    fn64: exp, pow and sqrt in float64, rounded to fp32 (nothing else changes).  kept: a list that receives, per pass, the filtered pixels
    whose sum of weights was not positive"""
    f = np.float32
    exp, power, sqrt = (_in64(np.exp), _in64(np.power), _in64(np.sqrt)) if fn64 else (np.exp, np.power, np.sqrt)
    rgb, var = rgb.astype(f), var.astype(f)
    filt = (pos[..., 3] != 0) & (light[..., 0] == 0) & (light[..., 1] == 0) & (light[..., 2] == 0)
    filt[image_rows:] = False
    a = np.maximum(dif[..., :3] + phg[..., :3], f(1e-3))
    yy = Y * Y
    with np.errstate(over="ignore", invalid="ignore"):
        uf = rgb / a
        s = ((yy[0] * var[..., 0]) / (a[..., 0] * a[..., 0]) + (yy[1] * var[..., 1]) / (a[..., 1] * a[..., 1])) + (yy[2] * var[..., 2]) / (a[..., 2] * a[..., 2])
    filt &= np.isfinite(uf).all(-1) & np.isfinite(s)              # a pixel whose demodulated colour or s is not finite is not filtered
    u = np.where(filt[..., None], uf, rgb)
    s = np.where(filt, s, f(0))
    xp, npl = pos[..., :3].astype(f), nrm[..., :3].astype(f)
    sxr = f(f(sigma_x) * f(radius))
    for i in range(levels):
        h = 1 << i
        gs = np.zeros_like(s); gw = np.zeros_like(s)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sq, ok = _shift(s, dy, dx); fq, _ = _shift(filt, dy, dx); ok &= fq
                k = f(f(B3[dx + 1]) * f(B3[dy + 1]))
                gs = np.where(ok, gs + k * sq, gs); gw = np.where(ok, gw + k, gw)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            gp = gs / gw
            lp = (Y[0] * u[..., 0] + Y[1] * u[..., 1]) + Y[2] * u[..., 2]
            dl = f(sigma_l) * sqrt(gp) + f(1e-10)
        sw = np.zeros_like(s); sr = np.zeros_like(s); sg = np.zeros_like(s); sb = np.zeros_like(s); ss = np.zeros_like(s)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                uq, ok = _shift(u, h * dy, h * dx); fq, _ = _shift(filt, h * dy, h * dx); ok &= fq
                sq, _ = _shift(s, h * dy, h * dx); xq, _ = _shift(xp, h * dy, h * dx); nq, _ = _shift(npl, h * dy, h * dx)
                k = f(f(B5[dx + 2]) * f(B5[dy + 2]))
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    lq = (Y[0] * uq[..., 0] + Y[1] * uq[..., 1]) + Y[2] * uq[..., 2]
                    el = np.abs(lp - lq) / dl
                    d = xq - xp
                    ex = np.abs((npl[..., 0] * d[..., 0] + npl[..., 1] * d[..., 1]) + npl[..., 2] * d[..., 2]) / sxr
                    nd = np.maximum(f(0), (npl[..., 0] * nq[..., 0] + npl[..., 1] * nq[..., 1]) + npl[..., 2] * nq[..., 2])
                    w = (k * exp(-el - ex)) * power(nd, f(sigma_n))
                    ok &= filt
                    w = np.where(ok, w, f(0))
                    sw = np.where(ok, sw + w, sw)
                    sr = np.where(ok, sr + w * uq[..., 0], sr); sg = np.where(ok, sg + w * uq[..., 1], sg); sb = np.where(ok, sb + w * uq[..., 2], sb)
                    ss = np.where(ok, ss + (w * w) * sq, ss)
        upd = filt & (sw > 0)
        if kept is not None:
            kept.append(filt & ~upd)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            un = np.stack([sr / sw, sg / sw, sb / sw], -1); sn = ss / (sw * sw)
        u = np.where(upd[..., None], un, u); s = np.where(upd, sn, s)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(filt[..., None], a * u, rgb).astype(f), filt


def rel_err(got, want):
    """the largest |got - want| / max(|want|, 1e-6 max |want|)"""
    floor = 1e-6 * float(np.abs(want).max())
    return float((np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want.astype(np.float64)), floor)).max())


_BARS = {}


def bars(case):
    """(sensitivity, distance to float64) of a case of CASES, from the references alone on host_inputs(): the largest relative difference
    between restate() and restate(fn64=True), and between restate() and statement64(), over the filtered image pixels with a finite
    composite.  The GPU's bar against restate() is max(1e-4, 8 x the first), against statement64() 4 x the second."""
    case = tuple(case)
    if case not in _BARS:
        c = make_case(*case)
        rgb, var = host_inputs(c)
        args = (rgb, var) + guides(c) + (c.light, RADIUS, c.H)
        a, filt = restate(*args)
        b, _ = restate(*args, fn64=True)
        d, _ = statement64(*args)
        m = filt[:c.H]
        _BARS[case] = (rel_err(a[:c.H][m], b[:c.H][m]), rel_err(a[:c.H][m], d[:c.H][m]))
    return _BARS[case]


# ---- include/evplp.h in float64
def _around(a, oy, ox, fill=0):
    """a[y + oy, x + ox] with `fill` outside the frame, by padding and slicing"""
    R, W = a.shape[:2]
    m = max(abs(oy), abs(ox))
    if m == 0:
        return a
    if abs(oy) >= R or abs(ox) >= W:
        return np.full_like(a, fill)
    p = np.pad(a, ((m, m), (m, m)) + ((0, 0),) * (a.ndim - 2), constant_values=fill)
    return p[m + oy:m + oy + R, m + ox:m + ox + W]


def statement64(rgb, var, pos, nrm, dif, phg, light, radius, image_rows, levels=5, sigma_luminance=4.0, sigma_normal=128.0, sigma_position=0.01):
    """evplp_denoise as include/evplp.h states it, every quantity in float64: (image (rows, W, 3) float64, the filtered pixels)"""
    y = np.array([0.2126, 0.7152, 0.0722])
    c, v = np.asarray(rgb, f64), np.asarray(var, f64)
    R, W = c.shape[:2]
    in_image = (np.arange(R) < image_rows)[:, None]
    F = in_image & (np.asarray(pos)[..., 3] != 0) & ~(np.asarray(light)[..., :3] != 0).any(-1)
    a = np.maximum(np.asarray(dif, f64)[..., :3] + np.asarray(phg, f64)[..., :3], 1e-3)
    with np.errstate(all="ignore"):
        u = c / a
        s = (y * y * v / (a * a)).sum(-1)
        # "A pixel whose demodulated colour or s is not finite (as the fp32 kernel computes them) is not filtered"
        F = F & np.isfinite(u.astype(f32)).all(-1) & np.isfinite(s.astype(f32))
    u = np.where(F[..., None], u, 0.0); s = np.where(F, s, 0.0)
    X = np.where(F[..., None], np.asarray(pos, f64)[..., :3], 0.0); n = np.where(F[..., None], np.asarray(nrm, f64)[..., :3], 0.0)
    b = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    b3 = np.array([0.25, 0.5, 0.25])
    for i in range(levels):
        h = 2 ** i
        num = np.zeros((R, W)); den = np.zeros((R, W))
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                Fq = _around(F, oy, ox, False)
                num += np.where(Fq, b3[ox + 1] * b3[oy + 1] * _around(s, oy, ox), 0.0); den += np.where(Fq, b3[ox + 1] * b3[oy + 1], 0.0)
        with np.errstate(all="ignore"):
            g = np.where(F, num / den, 0.0)
        l = u @ y
        sum_w = np.zeros((R, W)); sum_wu = np.zeros((R, W, 3)); sum_w2s = np.zeros((R, W))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = h * dy, h * dx
                Fq = _around(F, oy, ox, False) & F
                if not Fq.any():
                    continue
                uq, sq, Xq, nq = _around(u, oy, ox), _around(s, oy, ox), _around(X, oy, ox), _around(n, oy, ox)
                lum = np.abs(l - uq @ y) / (sigma_luminance * np.sqrt(g) + 1e-10)
                plane = np.abs((n * (Xq - X)).sum(-1)) / (sigma_position * radius)
                w = b[dx + 2] * b[dy + 2] * np.exp(-lum - plane) * np.maximum(0.0, (n * nq).sum(-1)) ** sigma_normal
                w = np.where(Fq, w, 0.0)
                sum_w += w; sum_wu += w[..., None] * uq; sum_w2s += w * w * sq
        ok = F & (sum_w > 0)
        with np.errstate(all="ignore"):
            u = np.where(ok[..., None], sum_wu / sum_w[..., None], u); s = np.where(ok, sum_w2s / (sum_w * sum_w), s)
    return np.where(F[..., None], a * u, c), F
