"""Hostile photon sets for the splat's binning, and their float64 reference (numpy only; shading_domain.photon_frag_f64 shades).

The shading of one (pixel, photon) fragment has its own tests (test_gpu_shading_domain.py).  This module is about WHICH pairs exist:
photon_rect, photon_reach2 / box_within, the tile boxes, the two-level binning with its segment overflow and its large-rectangle list,
the rank sort, the heavy list and the batch loop of the tile kernel (evplp_amd/csrc/kernels_splat.hip).  Every case is a synthetic
G-buffer seen through a camera of its own, a record set built by hand (flags, positions and predecessors are the test's to choose) and a
brute force over every (pixel, photon) pair in float64.

G-buffer.  A pixel's point is eye + depth(x, y) * dir(x, y) in float64, rounded to float32, with dir the ray through the pixel centre
under the jittered camera in the operation order of splat_tiles_kernel's ray (ndc = ((x + 0.5) / W * 2 - 1) - jitter; dir = s * ndc_x *
aspect * tan_half + u * ndc_y * tan_half + f): photon_rect relies on a pixel's point being seen through its own centre, and the float32
rounding of the point moves it by a few 1e-3 px at the coordinates used here, against photon_rect's guard of 1 / 32 px.  Normals and
reflectances come from four material classes by tile (all-Lambert tiles, two glossy classes, Lambert tiles with one glossy lane).
Background pixels carry the clear colour, position (0, 0, 0, 1).  Such a pixel is not on its own ray, so the product's screen rectangle
and the world-space rule |X - P| <= r may legitimately differ for a photon within r of the world origin: every photon here is kept farther
than r (1 + 1e-3) from the origin (the generators assert it), and no background pixel ever has an inside photon.

Records.  Photon i's predecessor is record i - 1, whatever that is.  Every record has a normal, a flux direction, reflectances, an
exponent and a lobe-selection probability of its own (the normal leans towards both neighbours in the buffer, so that most predecessors
face their photon), so a predecessor taken from the wrong slot changes mixPdfW, `alive` and brdf2 visibly.  Records that are not usable
carry a flux of 1e30.

Radius decisions.  A pair is radius-decided when |dist - r| >= 1e-4 r + 2^-21 pmag, pmag the largest absolute coordinate of the photon
and the pixel.  The first term is photon_frag_f64's margin.  The second: the kernel forms dv = P - X in float32 (each component rounded
to 2^-24 |dv_k| <= 2^-24 * 2 pmag at the very worst, exact when the two are within a factor of two of each other) and then dv . dv with
three more roundings of relative 2^-24 each; the distance so computed is off by at most about sqrt(3) 2^-24 pmag + 2 * 2^-24 r, and
2^-21 pmag = 8 * 2^-24 pmag covers that with a factor of about 4.  The generators re-draw any photon that has an undecided pair, so every
case's pair count is an exact integer that the oracle and the device must both meet.

Shading decisions.  A pixel is compared only if every one of its inside pairs is shading-decided (photon_frag_f64's `decided`); the host
test caps the undecided pixels at 2 % of the pixels that receive any photon, per case and mode.

Bar of a pixel with n inside photons: sum_k sd.bar(val_k, kappa_k, lam_k, K, True) + n 2^-24 sum_k |val_k| (the rule of
test_gather_whole_set: the bars of the terms, and 2^-24 of the running sum for each addition).

Predictions.  photon_rect and box_within are restated in float64 (rect64, reached) to say which path a photon takes -- LDS path (rectangle
of at most 3 x 3 tiles), large rectangle culled by the tile boxes (<= 64 tiles) or not culled (> 64 tiles), nothing on the screen -- and
which tiles get an entry.  A photon is re-drawn when its rectangle differs anywhere within +- 1 / 16 px of the guard, when its reached
tiles differ between a reach of r and of r plus twice photon_reach2's guard, or when its sphere's far end is within 1e-4 of the near
plane: the predictions then hold for any rounding the kernel's float32 arithmetic can have.
"""
import math
from types import SimpleNamespace

import numpy as np

import shading_domain as sd

MODES = (0, 3, 5)
CLAMP = 1.0e-12
BIN_GROUP = 256               # kBinGroup of kernels.h (EVPLP_BIN_CHUNKS = 1)
SEG_CAP = 4 * BIN_GROUP       # kSegCap
USABLE = 2                    # EVPLP_USABLE_PHOTON
GUARD_PX = 1.0 / 32.0         # photon_rect
FLIP_PX = 1.0 / 16.0
NEAR = 0.1
PATHS = ("none", "lds", "big_culled", "big_unculled")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


def _f32(v):
    return np.asarray(v, np.float32).astype(np.float64)


def default_stride(nrec, ntiles):
    """the bin_stride a context starts with (context.cpp: 8 x the mean occupancy, a power of two >= 64)"""
    mean, k = nrec * 2 // max(ntiles, 1), 64
    while k < 8 * mean and k < (1 << 20):
        k <<= 1
    return k


class Case:
    def __init__(self, name, W, H, origin, lookat, up, fovy_deg, jitter_px, radius, nlp, P, seed):
        self.name, self.W, self.H, self.nlp, self.P, self.seed = name, W, H, nlp, P, seed
        self.n = nlp * P
        self.cam = dict(origin=[float(np.float32(x)) for x in origin], lookat=[float(np.float32(x)) for x in lookat], up=[float(x) for x in up],
                        fovy=float(np.float32(math.radians(fovy_deg))), aspect=float(np.float32(W / H)))
        self.jitter = (float(np.float32(jitter_px[0] * 2.0 / W)), float(np.float32(jitter_px[1] * 2.0 / H)))      # NDC: one pixel = 2 / W
        self.set_radius(radius)
        self.tiles_x, self.tiles_y = (W + 7) // 8, (H + 7) // 8
        # camera_basis of context.cpp, in float32
        f32 = np.float32
        o, l, upv = (np.asarray(self.cam[k], f32) for k in ("origin", "lookat", "up"))
        nrm = lambda v: (v * (f32(1.0) / np.sqrt((v * v).sum(dtype=f32)))).astype(f32)
        f = nrm(l - o); s = nrm(np.cross(f, upv).astype(f32)); u = np.cross(s, f).astype(f32)
        self.eye, self.s, self.u, self.f = (np.asarray(v, np.float64) for v in (o, s, u, f))
        self.tan_half = float(np.tan(f32(self.cam["fovy"]) / f32(2.0)))
        self.aspect = self.cam["aspect"]
        self._refs = {}

    def set_radius(self, radius):
        self.r = float(np.float32(radius))
        self.pdf_mc = float(np.float32(1.0 / (math.pi * self.r * self.r)))

    # ---------------------------------------------------------------------------------------------------------- geometry
    def dir(self, px, py):
        """the ray through (fractional) pixel coordinates, pixel centres at integers, of the jittered camera; dir . f = 1"""
        px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
        ndx = ((px + 0.5) / self.W * 2.0 - 1.0) - self.jitter[0]
        ndy = ((py + 0.5) / self.H * 2.0 - 1.0) - self.jitter[1]
        dxs, dys = ndx * self.aspect * self.tan_half, ndy * self.tan_half
        return self.s * dxs[..., None] + self.u * dys[..., None] + self.f

    def at(self, px, py, depth):
        return self.eye + np.asarray(depth, np.float64)[..., None] * self.dir(px, py)

    def px_size(self, depth):
        return 2.0 * depth * self.tan_half / self.H

    def view(self, p):
        q = np.asarray(p, np.float64) - self.eye
        return q @ self.s, q @ self.u, q @ self.f

    def set_surface(self, depth_fn, background=None):
        """depth_fn(px, py) -> view depth, also off the screen (photons are placed on the surface there); background(x, y) -> the pixels that
        show nothing (photons may still lie where the surface would be)"""
        W, H = self.W, self.H
        self.depth_fn = depth_fn
        xs, ys = np.meshgrid(np.arange(W), np.arange(H))
        depth = depth_fn(xs.astype(np.float64), ys.astype(np.float64))
        bg = np.isnan(depth) if background is None else background(xs, ys)
        rng = np.random.RandomState(self.seed + 1)
        pos = np.zeros((H, W, 4), np.float32); nrm = np.zeros((H, W, 4), np.float32)
        dif = np.zeros((H, W, 4), np.float32); phg = np.zeros((H, W, 4), np.float32)
        pos[..., :3] = np.where(bg[..., None], 0.0, self.at(xs, ys, np.where(bg, 1.0, depth))).astype(np.float32); pos[..., 3] = 1.0
        tilt = rng.uniform(-1.0, 1.0, (H, W, 2))
        n = _unit(-self.f + 0.25 * (tilt[..., 0:1] * self.s + tilt[..., 1:2] * self.u))
        nrm[..., :3] = np.where(bg[..., None], 0.0, n)
        rd = (0.2 + 0.6 * rng.rand(H, W, 3)); rs = (0.1 + 0.4 * rng.rand(H, W, 3))
        cls = ((xs >> 3) + 2 * (ys >> 3)) % 4                # 0 all-Lambert, 1 glossy e = 20, 2 glossy e = 200, 3 Lambert with one glossy lane
        lane = (ys & 7) * 8 + (xs & 7)
        glossy = (cls == 1) | (cls == 2) | ((cls == 3) & (lane == 27))
        e = np.where(cls == 1, 20.0, np.where(cls == 2, 200.0, 5.0))
        dif[..., :3] = np.where(bg[..., None], 0.0, rd)
        phg[..., :3] = np.where((glossy & ~bg)[..., None], rs, 0.0)
        phg[..., 3] = np.where(glossy, e, 37.0)              # (a Lambert pixel keeps an exponent in the plane)
        self.gbuf = [pos, nrm, dif, phg]
        self.background = bg
        self.tile_class = cls
        self.pix = SimpleNamespace(pos=pos[..., :3].astype(np.float64).reshape(-1, 3), nrm=nrm[..., :3].astype(np.float64).reshape(-1, 3),
                                   rd=dif[..., :3].astype(np.float64).reshape(-1, 3), rs=phg[..., :3].astype(np.float64).reshape(-1, 3),
                                   e=phg[..., 3].astype(np.float64).reshape(-1))
        self.pix_mag = np.abs(self.pix.pos).max(-1)
        self.pix_tile = ((ys >> 3) * self.tiles_x + (xs >> 3)).reshape(-1)
        # float64 tile boxes over the in-image pixels, background included (splat_tile_box_kernel)
        nt = self.tiles_x * self.tiles_y
        self.box_lo = np.full((nt, 3), np.inf); self.box_hi = np.full((nt, 3), -np.inf)
        np.minimum.at(self.box_lo, self.pix_tile, self.pix.pos); np.maximum.at(self.box_hi, self.pix_tile, self.pix.pos)

    # ---------------------------------------------------------------------------------------------------------- predictions
    def rect64(self, p, guard=GUARD_PX):
        """photon_rect in float64: (tx0, tx1, ty0, ty1) or None"""
        r = self.r
        vx, vy, vz = self.view(p)
        zlo, zhi = max(vz - r, NEAR), min(vz + r, 100.0)
        if zlo > zhi:
            return None
        sx, sy = 1.0 / (self.aspect * self.tan_half), 1.0 / self.tan_half
        nx0 = min((vx - r) / zlo, (vx - r) / zhi) * sx + self.jitter[0]; nx1 = max((vx + r) / zlo, (vx + r) / zhi) * sx + self.jitter[0]
        ny0 = min((vy - r) / zlo, (vy - r) / zhi) * sy + self.jitter[1]; ny1 = max((vy + r) / zlo, (vy + r) / zhi) * sy + self.jitter[1]
        W, H = self.W, self.H
        fx0, fx1 = (nx0 * 0.5 + 0.5) * W - 0.5, (nx1 * 0.5 + 0.5) * W - 0.5
        fy0, fy1 = (ny0 * 0.5 + 0.5) * H - 0.5, (ny1 * 0.5 + 0.5) * H - 0.5
        clip = lambda v, hi: min(max(v, -1.0), float(hi))
        x0, x1 = max(math.ceil(clip(fx0 - guard, W)), 0), min(math.floor(clip(fx1 + guard, W)), W - 1)
        y0, y1 = max(math.ceil(clip(fy0 - guard, H)), 0), min(math.floor(clip(fy1 + guard, H)), H - 1)
        if x0 > x1 or y0 > y1:
            return None
        return (x0 >> 3, x1 >> 3, y0 >> 3, y1 >> 3)

    def reach_guard(self, p):
        return 1.0e-5 * self.r + 4.0e-6 * max(float(np.abs(p).max()), 1.0)

    def reached(self, p, rect, reach):
        """the tiles of `rect` whose box lies within `reach` of p (box_within)"""
        tx0, tx1, ty0, ty1 = rect
        t = (np.arange(ty0, ty1 + 1)[:, None] * self.tiles_x + np.arange(tx0, tx1 + 1)[None, :]).reshape(-1)
        d = np.maximum(np.maximum(self.box_lo[t] - p, p - self.box_hi[t]), 0.0)
        return t[~((d * d).sum(-1) > reach * reach)]

    def predict(self, p):
        """(path, tiles that get an entry, stable): stable = the prediction holds under the margins of the module docstring"""
        rect = self.rect64(p)
        stable = rect == self.rect64(p, GUARD_PX - FLIP_PX) == self.rect64(p, GUARD_PX + FLIP_PX)
        stable &= abs(self.view(p)[2] + self.r - NEAR) > 1.0e-4
        if rect is None:
            return "none", np.zeros(0, np.int64), stable, rect
        nx, ny = rect[1] - rect[0] + 1, rect[3] - rect[2] + 1
        g = self.reach_guard(p)
        if nx <= 3 and ny <= 3:
            path = "lds"
        elif nx * ny <= 64:
            path = "big_culled"
        else:
            path = "big_unculled"
        if path == "big_unculled":
            tiles = self.reached(p, rect, np.inf)
        else:
            tiles = self.reached(p, rect, self.r + g)
            stable &= len(self.reached(p, rect, self.r)) == len(tiles) == len(self.reached(p, rect, self.r + 2.0 * g))
        return path, tiles, stable, rect

    def near_pixels(self, p):
        """(indices of the pixels within r (1 + 1e-3) of p, their distances, every pair radius-decided?)"""
        dv = self.pix.pos - p
        dist = np.sqrt((dv * dv).sum(-1))
        margin = 1.0e-4 * self.r + 2.0 ** -21 * np.maximum(self.pix_mag, np.abs(p).max())
        return np.flatnonzero(dist <= self.r * (1.0 + 1.0e-3)), dist, bool((np.abs(dist - self.r) >= margin).all())

    # ---------------------------------------------------------------------------------------------------------- records
    def finish(self, spec, rounds=400):
        """spec: one entry per record, (draw(rng) -> position, usable, want, tag); want: None, a path name, "all" (every tile of the frame),
        ("tile", t) (an entry in tile t and nowhere else), "nothing" (no entry) or "no_pixels" (entries, and no pixel within r).  Draws every position, re-draws the usable photons that have an
        undecided pair, an unstable prediction or not what they want, then fills in the other fields of the records."""
        import oracle_api as oa
        assert len(spec) == self.n, (self.name, len(spec), self.n)
        rng = np.random.RandomState(self.seed)
        pos = np.zeros((self.n, 3), np.float64)
        self.usable = np.array([bool(s[1]) for s in spec])
        self.tags = [s[3] for s in spec]
        self.path = ["unused"] * self.n; self.entries = [np.zeros(0, np.int64)] * self.n; self.rect = [None] * self.n
        self._near = {}
        nt = self.tiles_x * self.tiles_y
        todo = list(range(self.n))
        for _ in range(rounds):
            again = []
            for i in todo:
                draw, usable, want, tag = spec[i]
                p = _f32(draw(rng)); pos[i] = p
                if not usable or i == 0:
                    continue
                assert np.sqrt((p * p).sum()) > self.r * (1.0 + 1.0e-3) * 1.5, (self.name, i, "a photon near the world origin")
                path, tiles, stable, rect = self.predict(p)
                idx, dist, rdec = self.near_pixels(p)
                ok = stable and rdec
                if want in PATHS:
                    ok &= path == want
                elif want == "all":
                    ok &= len(tiles) == nt
                elif want == "nothing":
                    ok &= len(tiles) == 0
                elif want == "no_pixels":
                    ok &= len(tiles) > 0 and not (dist <= self.r).any()
                elif want is not None:
                    ok &= list(tiles) == [want[1]]
                if not ok:
                    again.append(i); continue
                self.path[i], self.entries[i], self.rect[i] = path, tiles, rect
                self._near[i] = (idx, dist[idx] <= self.r)
            todo = again
            if not todo:
                break
        assert not todo, (self.name, "photons that never settled", todo[:8], [spec[i][3] for i in todo[:8]])
        self.photons = [i for i in range(1, self.n) if self.usable[i]]
        # the other fields: every record distinct, most predecessors facing their photon
        rec = np.zeros(self.n, dtype=oa.RECORD_DTYPE)
        nxt = _unit(np.roll(pos, -1, 0) - pos + 1e-30); prv = _unit(np.roll(pos, 1, 0) - pos + 1e-30)
        n = _unit(nxt + prv + 0.35 * rng.randn(self.n, 3))
        fd = _unit(n + 0.45 * rng.randn(self.n, 3))
        kind = np.arange(self.n) % 3
        rec["pos"] = pos; rec["normal"] = n; rec["flux_dir"] = fd
        rec["flux"] = np.where(self.usable[:, None], 0.5 + 1.5 * rng.rand(self.n, 3), sd.BIG)
        rec["rho_d"] = 0.2 + 0.6 * rng.rand(self.n, 3)
        rec["rho_s"] = np.where((kind != 0)[:, None], 0.1 + 0.4 * rng.rand(self.n, 3), 0.0)
        rec["phong_exp"] = np.where(kind == 1, 20.0, np.where(kind == 2, np.where(np.arange(self.n) % 2 == 0, 5.0, 60.0), 0.0))
        rec["p_select_lambert"] = np.where(kind == 0, 1.0, np.where(kind == 1, 0.3, 0.6))
        # `alive` is mixPdfW > 0.  Where the predecessor faces away from its photon (no Lambert term) and its lobe is d^e with d small, d^e is
        # 1e-60 in float64 and 0 in float32 (or a denormal that exp2 flushes): a discrete difference no margin of photon_frag_f64 covers.  Such a
        # predecessor takes the exponent 5 (d > 1e-5: d^5 > 1e-25).
        for i in range(1, self.n):
            if self.usable[i] and kind[i - 1] != 0:
                w12 = _unit(pos[i - 1] - pos[i])
                n1, f1 = rec["normal"][i - 1].astype(np.float64), rec["flux_dir"][i - 1].astype(np.float64)
                dp = float(np.dot(-w12, 2.0 * n1 * np.dot(n1, f1) - f1))
                if np.dot(n1, -w12) < 1.0e-3 and dp > 0.0 and dp ** float(rec["phong_exp"][i - 1]) < 1.0e-30:
                    rec["phong_exp"][i - 1] = 5.0
        rec["flags"] = np.where(self.usable, USABLE, 0)
        self.records = rec
        # predictions, summed
        self.entries_per_tile = np.zeros(nt, np.int64)
        for i in self.photons:
            self.entries_per_tile[self.entries[i]] += 1
        self.path_counts = {k: sum(self.path[i] == k for i in self.photons) for k in PATHS}
        groups = (self.n + BIN_GROUP - 1) // BIN_GROUP
        self.group_lds_entries = [sum(len(self.entries[i]) for i in self.photons if i // BIN_GROUP == g and self.path[i] == "lds") for g in range(groups)]
        # (the order in which a group's photons claim their slots is the hardware's: only a lower bound of the photons that overflow is predicted)
        self.seg_overflow_min = [max(0, -(-(e - SEG_CAP) // 9)) for e in self.group_lds_entries]
        self.big_predicted = sum(self.path[i] in ("big_culled", "big_unculled") for i in self.photons)
        self.pairs = int(sum(int(self._near[i][1].sum()) for i in self.photons))
        need = {(int(self.pix_tile[q]), i) for i in self.photons for q in self._near[i][0][self._near[i][1]]}
        self.tile_need = np.bincount(np.asarray([t for t, _ in need], np.int64), minlength=nt)       # photons with an inside pixel in the tile
        return self

    def params(self, mode):
        """keyword arguments of both frame_params constructors"""
        return dict(camera_pos=self.cam["origin"], mis_mode=mode, pdf_mc=self.pdf_mc, clamping_value=CLAMP, photon_radius=self.r, num_light_paths=self.nlp,
                    num_vpl_light_paths=self.nlp, photons_per_path=self.P, jitter=self.jitter)

    def inside_of(self, i):
        """flat indices of the pixels inside the radius of photon i"""
        idx, ins = self._near[i]
        return idx[ins]

    def describe(self, i):
        return f"{i}:{self.path[i]}" + (f"({self.tags[i]})" if self.tags[i] else "") + (" in a group whose segment overflows" if self.path[i] == "lds" and self.seg_overflow_min[i // BIN_GROUP] else "")

    # ---------------------------------------------------------------------------------------------------------- reference
    def reference(self, mode):
        """the float64 image and what its bar is made of: total [H, W, 3]; A = sum 2^-24 kappa |val|, L = sum 2^-22 lam |val|, S = sum |val|
        [H, W, 3]; n [H, W] inside photons; undecided [H, W]; by_pixel {flat pixel: [records]}"""
        if mode in self._refs:
            return self._refs[mode]
        HW = self.W * self.H
        total, A, L, S = (np.zeros((HW, 3)) for _ in range(4))
        n = np.zeros(HW, np.int64); und = np.zeros(HW, bool)
        by_pixel = {}
        fp = self.params(mode)
        for i in self.photons:
            idx, ins = self._near[i]
            if not ins.any():
                continue
            idx = idx[ins]
            pixel = SimpleNamespace(pos=self.pix.pos[idx], nrm=self.pix.nrm[idx], rd=self.pix.rd[idx], rs=self.pix.rs[idx], e=self.pix.e[idx])
            val, kappa, lam, decided, inside, rdec = sd.photon_frag_f64(mode, fp, pixel, self.records[i], self.records[i - 1])
            assert inside.all() and rdec.all(), (self.name, i)
            a = np.abs(val)
            total[idx] += val; A[idx] += 2.0 ** -24 * kappa * a; L[idx] += 2.0 ** -22 * lam[:, None] * a; S[idx] += a
            n[idx] += 1; und[idx] |= ~decided
            for q in idx:
                by_pixel.setdefault(int(q), []).append(i)
        sh = (self.H, self.W)
        ref = SimpleNamespace(total=total.reshape(sh + (3,)), A=A.reshape(sh + (3,)), L=L.reshape(sh + (3,)), S=S.reshape(sh + (3,)), n=n.reshape(sh),
                              undecided=und.reshape(sh), by_pixel=by_pixel)
        ref.compared = (ref.n > 0) & ~ref.undecided
        self._refs[mode] = ref
        return ref

    def bar(self, ref, K):
        return K * ref.A + ref.L + ref.n[..., None] * (1.0e-20 + 2.0 ** -24 * ref.S)

    def worst(self, ref, got, K, rows=None):
        """error / bar at its worst over the compared pixels (of the image rows `rows`), and where: (ratio, y, x, channel)"""
        sel = ref.compared if rows is None else ref.compared[rows]
        tot, bar = (ref.total, self.bar(ref, K)) if rows is None else (ref.total[rows], self.bar(ref, K)[rows])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(sel[..., None], np.abs(np.asarray(got, np.float64) - tot) / bar, 0.0)
        if not ratio.size:
            return 0.0, 0, 0, 0
        y, x, ch = np.unravel_index(int(ratio.argmax()), ratio.shape)
        return float(ratio.max()), int(y if rows is None else np.asarray(rows)[y]), int(x), int(ch)

    def blame(self, ref, y, x):
        """a pixel, its tile and the photons inside its radius with their predicted paths"""
        recs = ref.by_pixel.get(y * self.W + x, [])
        return f"pixel ({x}, {y}) of tile ({x >> 3}, {y >> 3}) [tile {(y >> 3) * self.tiles_x + (x >> 3)}], inside photons: " + ", ".join(self.describe(i) for i in recs)


# ---------------------------------------------------------------------------------------------------------------------- the cases
def _filler(c, lo=0.5, hi=0.9):
    """a record that is not a photon: somewhere in front of the surface (a plausible predecessor)"""
    def draw(rng):
        px, py = rng.uniform(0, c.W - 1), rng.uniform(0, c.H - 1)
        d = c.depth_fn(np.float64(px), np.float64(py))
        d = 10.0 if np.isnan(d) else float(d)
        return c.at(px, py, d * rng.uniform(lo, hi))
    return (draw, False, None, "")


def _on_surface(c, px, py, wiggle_px=0.0, lift=(-0.3, 0.3), want=None, tag=""):
    """a photon on the surface at pixel coordinates (px, py) (callables: drawn anew every time), lifted by lift x r towards the eye"""
    def draw(rng):
        x = px(rng) if callable(px) else px + wiggle_px * rng.uniform(-1, 1)
        y = py(rng) if callable(py) else py + wiggle_px * rng.uniform(-1, 1)
        return c.at(x, y, float(c.depth_fn(np.float64(x), np.float64(y))) - c.r * rng.uniform(*lift))
    return (draw, True, want, tag)


def _anywhere(c, want=None, tag="", lift=(-0.3, 0.3)):
    return _on_surface(c, lambda rng: rng.uniform(1.0, c.W - 2.0), lambda rng: rng.uniform(1.0, c.H - 2.0), want=want, tag=tag, lift=lift)


def _sprinkle(c, spec, count, rng, lo=1, hi=None, **kw):
    """`count` random photons on slots of spec[lo:hi] that still hold fillers"""
    free = [i for i in range(lo, hi if hi is not None else len(spec)) if not spec[i][1]]
    for i in rng.choice(free, size=count, replace=False):
        spec[int(i)] = _anywhere(c, **kw)


def seg_overflow():
    c = Case("seg_overflow", 96, 64, (3.0, 2.0, 8.0), (3.5, 2.25, -2.0), (0, 1, 0), 60.0, (0.7, -0.5), 1.0, 256, 4, 101)
    c.set_radius(6.9 * c.px_size(10.0))
    c.set_surface(lambda px, py: 10.0 + 0.0 * px)
    spec = [_filler(c) for _ in range(c.n)]
    for i in range(256, 512):
        spec[i] = _on_surface(c, lambda rng: rng.uniform(2.0, 93.0), lambda rng: rng.uniform(2.0, 61.0), want="lds", tag="dense group")
    rng = np.random.RandomState(1)
    for g in (0, 2, 3):
        _sprinkle(c, spec, 10, rng, max(1, g * 256), (g + 1) * 256)
    return c.finish(spec)


def big_rects():
    c = Case("big_rects", 132, 68, (-4.0, 6.0, 2.0), (-3.0, 5.5, -7.0), (0.1, 1, 0), 60.0, (-0.6, 0.8), 1.0, 128, 4, 202)
    c.set_surface(lambda px, py: 1.15 * (30.0 / 1.15) ** (np.clip(py, -8.0, 75.0) / 67.0) + 0.0 * px)
    spec = [_filler(c) for _ in range(c.n)]
    slots = np.random.RandomState(2).permutation(np.arange(1, c.n))
    wants = ["lds"] * 40 + ["big_culled"] * 30 + ["big_unculled"] * 12 + ["all"]
    for k, want in enumerate(wants):
        spec[int(slots[k])] = _anywhere(c, want=want, tag=want)
    return c.finish(spec, rounds=2000)


def near_plane():
    c = Case("near_plane", 96, 64, (-2.0, 1.5, 6.0), (-1.0, 1.0, -3.0), (0, 1, 0), 60.0, (0.9, 0.3), 0.15, 64, 4, 303)
    depth = lambda px, py: 0.1 + 0.3 * (px / 95.0) * (0.6 + 0.4 * py / 63.0)
    c.set_surface(depth)
    for k in range(200):                    # (the photon at the eye cannot be moved: the radius gives way, by 1e-4 at a time, until all its pairs are decided)
        c.set_radius(0.15 + 1.0e-4 * k)
        if c.near_pixels(c.eye)[2] and c.predict(c.eye)[2]:
            break
    else:
        raise AssertionError("near_plane: no radius decides the photon at the eye")

    def rel(vz, lateral, tag, want=None):
        def draw(rng):
            z = vz(rng) if callable(vz) else vz
            return c.eye + c.f * z + lateral * (rng.uniform(-1, 1) * c.s + rng.uniform(-1, 1) * c.u)
        return (draw, True, want, tag)
    spec = [_filler(c) for _ in range(c.n)]
    spec[7] = (lambda rng: c.eye.copy(), True, None, "at the eye")
    spec[19] = rel(lambda rng: rng.uniform(-0.03, -0.01), 0.01, "straddles the near plane")
    for k, i in enumerate((33, 34, 90, 140, 141, 250)):
        spec[i] = rel(lambda rng: rng.uniform(-c.r, NEAR - c.r - 0.002), 0.05, "behind", want="none")
    slots = [i for i in np.random.RandomState(3).permutation(np.arange(1, c.n)) if not spec[int(i)][1]][:30]
    for i in slots:
        spec[int(i)] = rel(lambda rng: rng.uniform(-c.r, NEAR + c.r), 0.2, "near")
    return c.finish(spec, rounds=2000)


def off_screen():
    c = Case("off_screen", 96, 64, (5.0, -3.0, 12.0), (5.0, -3.5, 2.0), (0, 1, 0), 60.0, (-0.8, -0.9), 1.0, 64, 4, 404)
    rp = 5.5
    c.set_radius(rp * c.px_size(10.0))
    c.set_surface(lambda px, py: 10.0 + 0.0 * px)
    W, H = c.W, c.H
    on = lambda x, y, tag, want=None, wiggle=0.02: _on_surface(c, x, y, wiggle_px=wiggle, lift=(0.0, 0.0), want=want, tag=tag)
    named = []
    for d in (0.3, 1.2, 3.0):
        named += [on(-rp + d, 10.3 + 9 * d, f"left {d}", wiggle=0.2), on(W - 1 + rp - d, 40.6 - 7 * d, f"right {d}", wiggle=0.2),
                  on(20.4 + 11 * d, -rp + d, f"bottom {d}", wiggle=0.2), on(70.7 - 13 * d, H - 1 + rp - d, f"top {d}", wiggle=0.2)]
    for a, tag in ((rp / math.sqrt(2.0) - 0.2, "corner single"), (rp / math.sqrt(2.0) - 1.0, "corner few")):
        named += [on(-a, -a, tag + " bl"), on(W - 1 + a, -a, tag + " br"), on(-a, H - 1 + a, tag + " tl"), on(W - 1 + a, H - 1 + a, tag + " tr")]
    # (the far end of a sphere just outside an edge still projects into the frame: a rectangle, and the cull leaves no entry)
    named += [on(-rp - 3.0, 30.0, "outside left", "nothing", 0.2), on(W + rp + 2.0, 30.0, "outside right", "nothing", 0.2), on(40.0, -rp - 3.0, "outside bottom", "nothing", 0.2),
              on(40.0, H + rp + 2.0, "outside top", "nothing", 0.2), on(-rp - 40.0, -rp - 40.0, "far outside", "none", 0.2)]
    spec = [_filler(c) for _ in range(c.n)]
    slots = np.random.RandomState(4).permutation(np.arange(1, c.n))
    for k, s in enumerate(named):
        spec[int(slots[k])] = s
    for k in range(len(named), len(named) + 20):
        spec[int(slots[k])] = _anywhere(c)
    return c.finish(spec)


def _borders(c, xs_border, ys_border, ragged_x, ragged_y, count_random, seed):
    """photons on the bucket borders, in the ragged tiles and in the four corners of the frame, and some anywhere"""
    W, H = c.W, c.H
    on = lambda x, y, tag: _on_surface(c, x, y, wiggle_px=0.3, tag=tag)
    named = []
    for xb in xs_border:
        for y in np.linspace(2.0, H - 2.5, 5):
            named.append(on(xb, float(y), f"bucket border x = {xb}"))
    for yb in ys_border:
        for x in np.linspace(3.0, W - 3.5, 7):
            named.append(on(float(x), yb, f"bucket border y = {yb}"))
    for xb in xs_border:
        for yb in ys_border:
            named.append(on(xb, yb, "bucket corner"))
    for k, x in enumerate(ragged_x):          # (one photon per ragged tile and position)
        for ty in range((H + 7) // 8):
            named.append(on(x, min(ty * 8 + 2.0 + 3.0 * k, H - 1.5), "ragged column"))
    for k, y in enumerate(ragged_y):
        for tx in range((W + 7) // 8):
            named.append(on(min(tx * 8 + 2.5 + 3.0 * k, W - 1.5), y, "ragged row"))
    for x, y in ((0.4, 0.5), (W - 1.4, 0.6), (0.5, H - 1.5), (W - 1.3, H - 1.4)):
        named.append(on(x, y, "frame corner"))
    spec = [_filler(c) for _ in range(c.n)]
    slots = np.random.RandomState(seed).permutation(np.arange(1, c.n))
    assert len(named) + count_random < c.n
    for k, s in enumerate(named):
        spec[int(slots[k])] = s
    for k in range(len(named), len(named) + count_random):
        spec[int(slots[k])] = _anywhere(c)
    return spec


def buckets_ragged_132x68():
    """17 x 9 tiles in 2 x 2 buckets of 16 x 8 tiles; the right column is 4 px wide, the top row 4 px high"""
    c = Case("buckets_ragged_132x68", 132, 68, (1.0, 7.0, 9.0), (2.0, 6.0, -1.0), (0, 1, 0.1), 60.0, (0.5, -0.7), 1.0, 128, 4, 505)
    c.set_radius(3.2 * c.px_size(10.0))
    c.set_surface(lambda px, py: 10.0 + 0.0 * px, background=lambda x, y: ((x >= 20) & (x < 29) & (y >= 10) & (y < 21)) | ((x >= 125) & (y >= 60) & (y < 66)))
    return c.finish(_borders(c, (127.5,), (63.5,), (129.3, 130.8), (65.2, 66.9), 40, 5))


def buckets_ragged_260x36():
    """33 x 5 tiles in 3 x 1 buckets (num_buckets = 3, padded to 4 in splat_bin_kernel); the right column is 4 px wide, the top tile row has 4 rows"""
    c = Case("buckets_ragged_260x36", 260, 36, (-6.0, -2.0, 5.0), (-6.5, -2.0, -5.0), (0, 1, 0), 40.0, (-0.4, 0.6), 1.0, 128, 4, 606)
    c.set_radius(3.2 * c.px_size(10.0))
    c.set_surface(lambda px, py: 10.0 + 0.0 * px)
    return c.finish(_borders(c, (127.5, 255.5), (), (257.2, 258.7), (32.6, 34.4), 40, 6))


RECORD_EDGES = (1, 255, 256, 257, 511, 512, 513, 749)


def record_edges():
    """750 records: three bin groups, the last with 238; photons at both ends of every 256-record chunk, record 0 flagged usable"""
    c = Case("record_edges", 96, 64, (2.0, 3.0, 15.0), (2.0, 3.0, 5.0), (0, 1, 0), 60.0, (0.3, 0.9), 1.0, 150, 5, 707)
    c.set_radius(5.0 * c.px_size(10.0))
    c.set_surface(lambda px, py: 10.0 + 0.0 * px)
    spec = [_filler(c) for _ in range(c.n)]
    for i in (0,) + RECORD_EDGES:
        spec[i] = _on_surface(c, 47.3, 31.6, wiggle_px=3.0, tag=f"record {i}")
    return c.finish(spec)


DENSE_TILES = ((2, 1, 70), (6, 4, 300), (9, 6, 1100))       # (tile column, tile row, photons)


def dense_bins():
    c = Case("dense_bins", 96, 64, (0.0, 4.0, 10.0), (0.0, 4.0, 0.0), (0, 1, 0), 60.0, (-0.2, 0.4), 1.0, 384, 4, 808)
    c.set_radius(2.94 * c.px_size(10.0))
    c.set_surface(lambda px, py: 10.0 + 0.0 * px)
    spec = [_filler(c) for _ in range(c.n)]
    slots = np.random.RandomState(8).permutation(np.arange(1, c.n))
    k = 0
    for tx, ty, count in DENSE_TILES:
        t = ty * c.tiles_x + tx
        for _ in range(count):
            spec[int(slots[k])] = _on_surface(c, (lambda rng, tx=tx: tx * 8 + rng.uniform(2.2, 4.8)), (lambda rng, ty=ty: ty * 8 + rng.uniform(2.2, 4.8)),
                                              lift=(-0.2, 0.2), want=("tile", t), tag=f"dense tile {t}")
            k += 1
    for _ in range(40):
        spec[int(slots[k])] = _anywhere(c); k += 1
    return c.finish(spec)


def depth_edges():
    """a foreground plane at depth 1 over the left half (4 px) of tile column 5, a wall at depth 30 behind it"""
    c = Case("depth_edges", 96, 64, (7.0, 1.0, 40.0), (7.5, 1.0, 0.0), (0, 1, 0), 60.0, (0.6, 0.6), 2.0, 64, 4, 909)
    fg = lambda px: (px >= 39.5) & (px < 43.5)
    c.set_surface(lambda px, py: np.where(fg(px), 1.0, 30.0) + 0.0 * py)
    spec = [_filler(c, 0.6, 0.9) for _ in range(c.n)]
    slots = np.random.RandomState(9).permutation(np.arange(1, c.n))
    k = 0
    for _ in range(30):
        spec[int(slots[k])] = _on_surface(c, lambda rng: rng.choice([rng.uniform(1.0, 38.0), rng.uniform(45.0, 94.0)]), lambda rng: rng.uniform(1.0, 62.0), tag="wall"); k += 1
    for _ in range(6):
        spec[int(slots[k])] = _on_surface(c, lambda rng: rng.uniform(40.0, 43.0), lambda rng: rng.uniform(1.0, 62.0), lift=(-0.05, 0.05), tag="foreground"); k += 1

    def floating(rng):
        return c.at(rng.uniform(40.5, 47.0), rng.uniform(1.0, 62.0), rng.uniform(1.0 + c.r * 1.1, 30.0 - c.r * 1.1))
    for _ in range(12):
        spec[int(slots[k])] = (floating, True, "no_pixels", "floating"); k += 1
    return c.finish(spec)


def far_coordinates():
    """the borders-and-corners photons of buckets_ragged around coordinates of order 1e3, radius 0.05"""
    eye = np.array([1000.5, -800.25, 600.75])
    c = Case("far_coordinates", 96, 64, eye, eye + np.array([0.3, -0.2, -1.0]), (0, 1, 0), 60.0, (0.8, -0.3), 0.05, 64, 4, 1010)
    c.set_surface(lambda px, py: 1.0 + 0.0 * px)
    return c.finish(_borders(c, (31.5, 63.5), (31.5,), (94.2,), (62.8,), 40, 10), rounds=4000)


BUILDERS = dict(seg_overflow=seg_overflow, big_rects=big_rects, near_plane=near_plane, off_screen=off_screen, buckets_ragged_132x68=buckets_ragged_132x68,
                buckets_ragged_260x36=buckets_ragged_260x36, record_edges=record_edges, dense_bins=dense_bins, depth_edges=depth_edges,
                far_coordinates=far_coordinates)
NAMES = tuple(BUILDERS)
_cases = {}


def case(name):
    """the case, built once per process"""
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]
