"""Hostile ray batches for evplp_trace_closest / evplp_trace_occluded and their references (no GPU needed to build them): far origins,
scaled directions, oblique and flat scenes.  Shared by test_ray_query_hostile_host.py (the references alone) and
test_gpu_ray_query_hostile.py (the device against them).

The reference of every valid ray is the brute force: evo_closest_brute / evo_occluded_brute, the triangle test over every triangle.  The
triangle test can accept a point that no conservative box test is obliged to find, and a far origin widens that, so
a condition on the references alone says which rays are compared byte for byte.  A ray is DECIDABLE if the brute force reports a miss, or
if the exact ray -- its fp32 origin and direction taken as reals, the test done in float64 -- crosses the unpadded axis-aligned box of
the brute-force winner within (tmin, tmax); for occlusion the winner is evo_closest_brute's with filter 0 and the same bounds.  Every
other ray is SET ASIDE: the device's answer for it only has to be a triangle evo_tri_test accepts with the reported t bits, or a miss.
At most CAP of any (scene, kind) may be set aside."""
import ctypes as C

import numpy as np

import oracle_api as oa
import scenes
from test_gpu_ray_query import INVALID_KINDS, has_area, invalid_rays, on_triangle, rays_of, unit

F = np.float32
D = np.float64
W, H = 64, 48
N_RAYS = 4096
CAP = 0.005
FAR_R = (1e2, 1e3, 1e4)
SCALES = (-100, -60, 60, 100)
# a direction whose largest component lies outside [2^-64, 2^64] is an invalid ray (include/evplp.h): the 2^+-100 copies join the invalid kinds
HOSTILE_INVALID = tuple(f"scaled d 2^{e}" for e in SCALES if abs(e) > 64)
ULP = 2.0 ** -24
K_MAX = 20.0              # targets near a vertex or an outline lie k * 2^-24 * R * S inside it, k uniform in [0, K_MAX]
N_FAR, N_SCALED, N_PLANE, N_EXACT = 600, 200, 286, 20
SCENES = ("soup", "soup far away", "soup 1e-3", "soup 1e3", "flat", "room")


def make_scene(name):
    if name == "soup":
        return scenes.oblique_soup(seed=5, aspect=W / H)
    if name == "soup far away":
        return scenes.moved(scenes.oblique_soup(seed=5, aspect=W / H), 1.0, (4000.0, -3000.0, 2500.0))
    if name == "soup 1e-3":
        return scenes.moved(scenes.oblique_soup(seed=5, aspect=W / H), 1e-3)
    if name == "soup 1e3":
        return scenes.moved(scenes.oblique_soup(seed=5, aspect=W / H), 1e3)
    if name == "flat":
        return scenes.flat_scene(seed=2, aspect=W / H)
    if name == "room":
        return scenes.box_room(seed=3, n_boxes=6, tess=2, aspect=W / H)
    raise KeyError(name)


def scene_extent(V):
    """(lo, hi, S) over the triangles that have area, S as bvh_pad computes it (bvh_build.cpp): the larger of the box's diagonal and the
    largest coordinate magnitude"""
    P = V[has_area(V)].reshape(-1, 3)
    lo, hi = P.min(axis=0), P.max(axis=0)
    diag = np.sqrt(((hi - lo).astype(F) ** 2).sum(dtype=F))
    return lo.astype(D), hi.astype(D), float(max(diag, np.abs(lo).max(), np.abs(hi).max()))


def outline_edges(V):
    """(triangle, corner a, corner b) of every edge of a triangle with area that no coplanar triangle shares: the outline of a face"""
    valid = has_area(V)
    P = V.reshape(-1, 3, 3).astype(D)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    owners = {}
    for t in np.nonzero(valid)[0]:
        for a in range(3):
            key = frozenset((V[t, 3 * a:3 * a + 3].tobytes(), V[t, 3 * ((a + 1) % 3):3 * ((a + 1) % 3) + 3].tobytes()))
            owners.setdefault(key, []).append((t, a))
    scale = np.abs(P).max() + 1.0
    out = []
    for lst in owners.values():
        for t, a in lst:
            shared = False
            for u, _ in lst:
                if u != t and np.linalg.norm(np.cross(nrm[t], nrm[u])) < 1e-6 and abs((P[u, 0] - P[t, 0]) @ nrm[t]) < 1e-6 * scale:
                    shared = True
            if not shared:
                out.append((t, a, (a + 1) % 3))
    return np.array(sorted(out), np.int64)


def crosses_box(rays, lo, hi):
    """the exact ray (fp32 origin and direction as reals, float64 arithmetic) against the boxes [lo, hi], one per ray, within (tmin, tmax)"""
    o, d = rays[:, 0:3].astype(D), rays[:, 4:7].astype(D)
    tn, tf = rays[:, 3].astype(D).copy(), rays[:, 7].astype(D).copy()
    ok = np.ones(rays.shape[0], bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(3):
            par = d[:, k] == 0.0
            t0, t1 = (lo[:, k] - o[:, k]) / d[:, k], (hi[:, k] - o[:, k]) / d[:, k]
            a, b = np.minimum(t0, t1), np.maximum(t0, t1)
            ok &= np.where(par, (lo[:, k] <= o[:, k]) & (o[:, k] <= hi[:, k]), True)
            tn = np.where(par, tn, np.maximum(tn, a)); tf = np.where(par, tf, np.minimum(tf, b))
    return ok & (tn <= tf)


class Hostile:
    """one scene's batch (kinds: the names to build, with their counts) with the brute-force answers and the rays set aside"""

    def __init__(self, sd, seed=11, n_rays=N_RAYS, far=FAR_R, scaled=True, plane=None, classic_invalid=True):
        rng = self.rng = np.random.RandomState(seed)
        self.sd, self.osc = sd, oa.Scene(sd)
        V = self.V = sd.triangle_soup()[0]
        self.light = (sd.light_first, sd.light_count)
        self.area = has_area(V)
        self.P = V.reshape(-1, 3, 3).astype(D)
        self.lo, self.hi, self.S = scene_extent(V)
        self.tris = np.nonzero(self.area)[0]
        self.outline = outline_edges(V)
        self.height = self._heights()
        planted = getattr(sd, "planted", None)
        if plane is None:
            plane = planted is None
        parts, kinds = [], []

        def add(kind, r):
            parts.append(r.astype(F)); kinds.extend([kind] * r.shape[0])
        n_fixed = (len(INVALID_KINDS) if classic_invalid else 0) + len(far) * N_FAR + (len(SCALES) * N_SCALED if scaled else 0) + (N_PLANE if plane else 0)
        near = self.near_rays(n_rays - n_fixed)
        add("near", near)
        for R in far:
            add(f"far {R:g}", self.far_rays(R, N_FAR))
        if scaled:
            # the first near rays, every direction as a unit vector: a d = target - o of the 1e-3 soup is itself 2^-8 and smaller, and
            # what is asked of 2^+-60 is that it stays inside the range evplp.h accepts whatever the scene's size
            base = near[:N_SCALED].copy(); base[:, 3] = 0.0; base[:, 7] = 3.0e38
            base[:, 4:7] = (base[:, 4:7].astype(D) / np.linalg.norm(base[:, 4:7].astype(D), axis=1, keepdims=True)).astype(F)
            self.scaled_base = base
            for e in SCALES:
                r = base.copy(); r[:, 4:7] = np.ldexp(base[:, 4:7], e)
                add(f"scaled d 2^{e}", r)
        if plane:
            add("in plane", self.plane_rays(N_PLANE))
        rays = np.concatenate(parts)
        n_inv = len(INVALID_KINDS) if classic_invalid else 0
        assert rays.shape[0] == n_rays - n_inv, rays.shape
        at = np.array([137, 511, 1026, 1600, 2047, 2500, 3001, 3333, 3800, 4000])[:n_inv]
        keep = np.ones(n_rays, bool); keep[at] = False
        self.rays = np.zeros((n_rays, 8), F); self.rays[keep] = rays
        self.kinds = np.empty(n_rays, object); self.kinds[keep] = kinds
        if n_inv:
            self.rays[at] = invalid_rays(); self.kinds[at] = INVALID_KINDS
        self.n = n_rays
        # rays the device must refuse (triangle -2, byte 2): the existing test's ten kinds and the directions beyond 2^+-64
        self.valid = keep & ~np.isin(self.kinds, HOSTILE_INVALID)
        largest = np.abs(self.rays[:, 4:7]).max(axis=1)
        assert np.array_equal(self.valid[keep], ((largest >= F(2.0 ** -64)) & (largest <= F(2.0 ** 64)))[keep]), "the kinds refused are those the header's rule refuses"
        self.invalid = np.nonzero(~self.valid)[0]
        # references: the brute force for every ray a triangle test can be asked about (the classic invalid ones hold NaNs: left out)
        self.brute, self.aside = {}, {}
        hit_dtype = [("t", F), ("beta", F), ("gamma", F), ("triangle", np.int32)]
        v = np.ascontiguousarray(self.rays[keep])
        for filt in (0, 1, 2):
            e = np.zeros(n_rays, hit_dtype); e[keep] = self.osc.closest_brute(v, filt); e["triangle"][at] = -2
            self.brute[filt] = e
            self.aside[filt] = self._set_aside(e["triangle"]) & keep
        self.brute_occluded = np.full(n_rays, 2, np.uint8); self.brute_occluded[keep] = self.osc.occluded_brute(v)
        self.aside_occluded = self.aside[0]
        # what the device must return: the brute force, and for the rays it must refuse (-2, 0, 0, 0) / 2
        self.closest = {}
        for filt in (0, 1, 2):
            e = self.brute[filt].copy(); e[~self.valid] = np.zeros(1, hit_dtype)[0]; e["triangle"][~self.valid] = -2
            self.closest[filt] = e
        self.occluded = self.brute_occluded.copy(); self.occluded[~self.valid] = 2

    # ---- geometry
    def _heights(self):
        """the smallest height of every triangle (0 for one without area)"""
        P = self.P
        a2 = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
        longest = np.maximum(np.maximum(np.linalg.norm(P[:, 1] - P[:, 0], axis=1), np.linalg.norm(P[:, 2] - P[:, 1], axis=1)), np.linalg.norm(P[:, 0] - P[:, 2], axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(longest > 0, a2 / longest, 0.0)

    def free_points(self, n):
        return self.lo + self.rng.uniform(0.05, 0.95, size=(n, 3)) * (self.hi - self.lo)

    def interior(self, tri):
        n = len(tri)
        b, g = self.rng.uniform(0.1, 0.45, n), self.rng.uniform(0.1, 0.45, n)
        P = self.P[tri]
        return P[:, 0] + b[:, None] * (P[:, 1] - P[:, 0]) + g[:, None] * (P[:, 2] - P[:, 0])

    def near_vertex(self, tri, delta):
        """delta inside a corner, towards the centroid; never further than a fifth of the way to it"""
        P = self.P[tri]
        v = P[np.arange(len(tri)), self.rng.randint(0, 3, len(tri))]
        to = P.mean(axis=1) - v
        L = np.linalg.norm(to, axis=1)
        return v + (np.minimum(delta, 0.2 * L) / L)[:, None] * to

    def near_outline(self, edges, delta):
        """delta inside an outline edge, at right angles to it in the triangle's plane; never further than a fifth of the height over it"""
        n = len(edges)
        P = self.P[edges[:, 0]]
        a, b = P[np.arange(n), edges[:, 1]], P[np.arange(n), edges[:, 2]]
        c = P[np.arange(n), 3 - edges[:, 1] - edges[:, 2]]
        e = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
        up = (c - a) - ((c - a) * e).sum(axis=1, keepdims=True) * e
        h = np.linalg.norm(up, axis=1)
        s = self.rng.uniform(0.1, 0.9, n)
        return a + s[:, None] * (b - a) + (np.minimum(delta, 0.2 * h) / h)[:, None] * up

    def big_enough(self, need):
        """the triangles whose smallest height is at least `need`; where fewer than 24 are, the 24 of the largest such height"""
        idx = self.tris[self.height[self.tris] >= need]
        if len(idx) < 24:
            idx = self.tris[np.argsort(self.height[self.tris])[-24:]]
        return idx

    # ---- kinds
    def near_rays(self, n):
        """origins inside the scene's box.  Aimed (d = target - o, or that as a unit vector) at interior points, corners, points on
        edges, the fan's hub and the tie pairs, 60 from origins exactly on a surface; the rest are random unit directions with short far bounds.  tmin alternates 0 and 1e-4."""
        rng, sd = self.rng, self.sd
        planted = getattr(sd, "planted", None)
        n_rand = n // 5
        n_aim = n - n_rand
        tri = rng.choice(self.tris, n_aim)
        target = self.interior(tri)
        o = self.free_points(n_aim)
        q0 = N_SCALED
        if planted is not None:
            ties = np.array([planted["ties"][0][0], planted["ties"][1][0]])[rng.randint(0, 2, 80)]
            target[0:80] = self.interior(ties)
            o[0:80] = np.clip(target[0:80] + rng.uniform(-0.09, 0.09, (80, 3)) * self.S, self.lo, self.hi)      # (from nearby: little of the soup in between)
            target[q0:q0 + 40] = sd.fan_hub.astype(D)
            q0 += 40
        # 60 origins exactly on a surface with a random direction: from a wall of a closed room half of them leave the scene
        st = rng.choice(self.tris, 60)
        o[80:140] = on_triangle(self.V, st, rng.uniform(0.1, 0.45, 60).astype(F), rng.uniform(0.1, 0.45, 60).astype(F))
        target[80:140] = o[80:140].astype(F).astype(D) + unit(rng, 60).astype(D)
        # The first N_SCALED rays (the tie pairs, the surface origins and interior points) are the base of the scaled kinds.  Behind them the rays aimed exactly
        # at a corner (the hub, N_EXACT random ones) or at a point on the edge p0 p1 (N_EXACT).  A ray aimed exactly at the border of an
        # axis-aligned face passes, as a real line, on either side of it: about a quarter of these are set aside in the room, which
        # bounds how many a kind can hold under the cap
        q = N_EXACT
        P = self.P[tri[q0:q0 + q]]
        target[q0:q0 + q] = P[np.arange(q), rng.randint(0, 3, q)]
        s = rng.uniform(0.0, 1.0, q); P = self.P[tri[q0 + q:q0 + 2 * q]]
        target[q0 + q:q0 + 2 * q] = P[:, 0] + s[:, None] * (P[:, 1] - P[:, 0])
        o = o.astype(F); target = target.astype(F)
        d = (target - o).astype(F)
        far = np.full(n_aim, 3.0e38, F)
        half = np.arange(n_aim) % 2 == 1
        L = np.linalg.norm(d.astype(D), axis=1)
        d[half] = (d[half].astype(D) / L[half, None]).astype(F)
        short = np.arange(n_aim) % 7 == 3                                                                # some far bounds are short: before or just behind the target
        far[short] = (np.where(half, L, 1.0) * rng.uniform(0.5, 1.5, n_aim)).astype(F)[short]
        aimed = rays_of(o, d, 0.0, far)
        rnd = rays_of(self.free_points(n_rand).astype(F), unit(rng, n_rand), 0.0, (rng.uniform(0.02, 0.8, n_rand) * self.S).astype(F))
        r = np.concatenate([aimed, rnd])
        r[1::2, 3] = F(1e-4)
        return r

    def far_rays(self, R, n):
        """origins R S from the target in a random direction; half with d = target - o (t about 1), half with a unit d (t about R S).
        A third of the targets are interior points, a third lie k 2^-24 R S inside a corner, a third the same distance inside an outline edge."""
        rng = self.rng
        dist = R * self.S
        third = n // 3
        delta = rng.uniform(0.0, K_MAX, n) * ULP * dist
        big = self.big_enough(4.0 * K_MAX * ULP * dist)
        t_in = self.interior(rng.choice(big, third))
        t_v = self.near_vertex(rng.choice(big, third), delta[:third])
        ol = self.outline[np.isin(self.outline[:, 0], big)]
        t_o = self.near_outline(ol[rng.randint(0, len(ol), n - 2 * third)], delta[third:n - third])
        target = np.concatenate([t_in, t_v, t_o])
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = (target + dist * u).astype(F)
        d = (target.astype(F) - o).astype(F)
        half = np.arange(n) % 2 == 1
        d[half] = (d[half].astype(D) / np.linalg.norm(d[half].astype(D), axis=1, keepdims=True)).astype(F)
        r = rays_of(o, d, 0.0, 3.0e38)
        r[1::4, 3] = F(1e-4)
        # every eighth far bound ends 5 % short of the target (the scene is at most a hundredth of the way across): a miss by the far bound
        t_target = np.where(half, np.linalg.norm(target - o.astype(D), axis=1), 1.0)
        r[5::8, 7] = (0.95 * t_target).astype(F)[5::8]
        self.far_target = getattr(self, "far_target", {}); self.far_target[R] = np.repeat(["interior", "vertex", "outline"], [third, third, n - 2 * third])
        return r

    def plane_rays(self, n):
        """origins exactly on the plane of an axis-aligned face (inside the face), directions exactly in that plane: one zero component,
        for a third of them two (axis-parallel), the zeros of either sign"""
        rng, V = self.rng, self.V
        faces = [(t, k) for t in self.tris for k in range(3) if V[t, k] == V[t, 3 + k] == V[t, 6 + k]]
        assert len(faces) >= 16
        pick = [faces[i] for i in rng.randint(0, len(faces), n)]
        tri, axis = np.array([p[0] for p in pick]), np.array([p[1] for p in pick])
        o = on_triangle(V, tri, rng.uniform(0.1, 0.45, n).astype(F), rng.uniform(0.1, 0.45, n).astype(F))
        d = unit(rng, n)
        d[np.arange(n), axis] = 0.0
        par = np.arange(n) % 3 == 0
        d[par, (axis[par] + 1) % 3] = 0.0
        d[par, (axis[par] + 2) % 3] = rng.choice([-1.0, 1.0, 2.5, -0.5], int(par.sum())).astype(F)
        neg = (d == 0.0) & (rng.rand(n, 3) < 0.5)
        d[neg] = F(-0.0)
        r = rays_of(o, d, 1e-4, 3.0e38)
        r[1::2, 3] = 0.0
        r[2::6, 7] = rng.uniform(0.05, 0.5, len(r[2::6])).astype(F)          # (short far bounds: a closed room lets no other ray miss)
        return r

    # ---- the condition on the references
    def _set_aside(self, winner):
        hit = winner >= 0
        w = np.where(hit, winner, 0)
        lo, hi = self.P[w].min(axis=1), self.P[w].max(axis=1)
        with np.errstate(invalid="ignore"):
            return hit & ~crosses_box(self.rays, lo, hi)

    def share_aside(self, kind):
        m = self.kinds == kind
        return max(float(self.aside[f][m].mean()) for f in (0, 1, 2))

    # ---- the device against the references
    def check_closest(self, hits, filt, what):
        want, aside = self.closest[filt], self.aside[filt] & self.valid
        assert hits.dtype.itemsize == 16 and hits.shape == (self.n,)
        bad = [i for i in np.nonzero(~aside)[0] if hits[i].tobytes() != want[i].tobytes()]
        by_kind = {}
        for i in bad:
            by_kind[self.kinds[i]] = by_kind.get(self.kinds[i], 0) + 1
        assert not bad, f"{what}: {len(bad)} rays differ from the brute force {by_kind}, first {[(i, self.kinds[i], hits[i], want[i]) for i in bad[:4]]}"
        L = self.osc.lib
        t, b, g = C.c_float(), C.c_float(), C.c_float()
        for i in np.nonzero(aside)[0]:                      # (set aside: any triangle the test accepts with the reported t bits, or a miss)
            k, r = int(hits["triangle"][i]), self.rays[i]
            if k == -1:
                continue
            assert 0 <= k < self.V.shape[0] and self.area[k], (what, i, k)
            c = [np.ascontiguousarray(self.V[k, j:j + 3]) for j in (0, 3, 6)]
            o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
            assert L.evo_tri_test(oa.ptr(c[0]), oa.ptr(c[1]), oa.ptr(c[2]), oa.ptr(o), oa.ptr(d), float(r[3]), float(r[7]), C.byref(t), C.byref(b), C.byref(g)), (what, i)
            assert F(t.value).tobytes() == hits["t"][i].tobytes(), (what, i)

    def check_occluded(self, out, what):
        assert out.dtype == np.uint8 and out.shape == (self.n,)
        aside = self.aside_occluded & self.valid
        bad = np.nonzero((out != self.occluded) & ~aside)[0]
        by_kind = {}
        for i in bad:
            by_kind[self.kinds[i]] = by_kind.get(self.kinds[i], 0) + 1
        assert len(bad) == 0, f"{what}: {len(bad)} rays differ from evo_occluded_brute {by_kind}, first {[(i, self.kinds[i], out[i], self.occluded[i]) for i in bad[:4]]}"
        assert (out[aside] < 2).all()
