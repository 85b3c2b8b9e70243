"""Ray queries on the device against the oracle: evplp_trace_closest / evplp_trace_occluded, their device forms and evplp_triangle_info.

The reference is the oracle scene built from the same triangles: evo_closest and evo_occluded_brute per ray, and for 256 rays of the batch a
brute force that loops evo_tri_test over every triangle with the tie rule (smallest t, then lowest index).  DESIGN.md section 2 has the one
known exception: a segment within about a degree of a triangle's plane can be accepted by the triangle test outside every padded box, so
two trees may differ on it.  It is handled by a condition on the references alone: a ray on which evo_closest and the brute force disagree
(for occlusion: evo_occluded and evo_occluded_brute) is SET ASIDE, and the device's answer for it only has to be a triangle evo_tri_test
accepts with the reported t bits.  At most 0.5 % of a batch may be set aside; on scenes.box_room with these seeds none is.  Every other
ray is compared byte for byte: triangle, t, beta, gamma."""
import copy
import ctypes as C

import numpy as np
import pytest

import oracle_api as oa
import scenes
import walk_replay as wr

pytestmark = pytest.mark.gpu

F = np.float32
W, H, NP, P = 64, 48, 32, 4          # the contexts' frame: no pass is rendered here
N_RAYS, N_BRUTE, N_TMAX = 4096, 256, 128
BUILDERS = {0: "lbvh", 1: "sah", 2: "sbvh", 3: "gpu", 4: "ploc"}
INVALID_KINDS = ("nan origin", "inf origin", "nan direction", "inf direction", "zero direction", "nan tmin", "inf tmin", "nan tmax", "inf tmax", "tmin > tmax")


def say(*a):
    print("[ray query]", *a, flush=True)


def rays_of(o, d, tmin, tmax):
    o, d = np.asarray(o, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    r = np.zeros((o.shape[0], 8), F)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def free_points(rng, n):
    """points inside the room [0, 10] x [0, 8] x [0, 5] (some lie inside a box: rays may start anywhere)"""
    return (rng.uniform(0.05, 0.95, size=(n, 3)) * np.array([10.0, 8.0, 5.0])).astype(F)


def on_triangle(V, tri, b, g):
    """p0 + b (p1 - p0) + g (p2 - p0) in fp32: a coordinate the three corners share stays exactly theirs"""
    p0, p1, p2 = V[tri, 0:3], V[tri, 3:6], V[tri, 6:9]
    return (p0 + b[:, None] * (p1 - p0) + g[:, None] * (p2 - p0)).astype(F)


def oracle_closest(osc, rays, filt):
    """evo_closest per ray as the hits the device must report (a miss: t = tmax, beta = gamma = 0, triangle -1)"""
    L = osc.lib
    out = np.zeros(rays.shape[0], [("t", F), ("beta", F), ("gamma", F), ("triangle", np.int32)])
    t, b, g = C.c_float(), C.c_float(), C.c_float()
    for i, r in enumerate(rays):
        o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
        tri = L.evo_closest(osc.h, oa.ptr(o), oa.ptr(d), float(r[3]), float(r[7]), filt, C.byref(t), C.byref(b), C.byref(g))
        out[i] = (t.value, b.value, g.value, tri) if tri >= 0 else (r[7], 0.0, 0.0, -1)
    return out


def oracle_occluded(osc, rays, brute=True):
    L = osc.lib
    fn = L.evo_occluded_brute if brute else L.evo_occluded
    out = np.zeros(rays.shape[0], np.uint8)
    for i, r in enumerate(rays):
        o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
        out[i] = fn(osc.h, oa.ptr(o), oa.ptr(d), float(r[3]), float(r[7]))
    return out


def has_area(V):
    """the oracle's tri_valid in fp32"""
    cr = np.cross((V[:, 3:6] - V[:, 0:3]).astype(F), (V[:, 6:9] - V[:, 0:3]).astype(F)).astype(F)
    a = np.sqrt((cr * cr).sum(axis=1, dtype=F))
    return (a > 0) & np.isfinite(a)


def brute_table(osc, V, rays):
    """evo_tri_test of every (ray, triangle) with the ray's tmin and the walks' far bound 3e38: accepted, t, beta, gamma"""
    L = osc.lib
    n, m = rays.shape[0], V.shape[0]
    ok = np.zeros((n, m), bool); T = np.zeros((n, m), F); B = np.zeros((n, m), F); G = np.zeros((n, m), F)
    t, b, g = C.c_float(), C.c_float(), C.c_float()
    keep = [np.ascontiguousarray(V[k, j:j + 3]) for k in range(m) for j in (0, 3, 6)]        # (the pointers below point into these)
    corners = [(oa.ptr(keep[3 * k]), oa.ptr(keep[3 * k + 1]), oa.ptr(keep[3 * k + 2])) for k in range(m)]
    valid = has_area(V)
    for i, r in enumerate(rays):
        o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
        po, pd, tmin = oa.ptr(o), oa.ptr(d), float(r[3])
        for k in range(m):
            if valid[k] and L.evo_tri_test(corners[k][0], corners[k][1], corners[k][2], po, pd, tmin, 3.0e38, C.byref(t), C.byref(b), C.byref(g)):
                ok[i, k], T[i, k], B[i, k], G[i, k] = True, t.value, b.value, g.value
    return ok, T, B, G


def brute_closest(table, rays, light, filt):
    """the tie rule over the table: among accepted triangles with t < tmax the smallest t, then the lowest index"""
    ok, T, B, G = table
    first, count = light
    idx = np.arange(ok.shape[1])
    is_light = (idx >= first) & (idx < first + count)
    allowed = np.ones_like(is_light) if filt == 0 else ~is_light if filt == 1 else is_light
    out = np.zeros(rays.shape[0], [("t", F), ("beta", F), ("gamma", F), ("triangle", np.int32)])
    for i, r in enumerate(rays):
        cand = np.nonzero(ok[i] & allowed & (T[i] < r[7]))[0]
        if len(cand) == 0:
            out[i] = (r[7], 0.0, 0.0, -1)
            continue
        k = cand[np.lexsort((cand, T[i, cand]))[0]]
        out[i] = (T[i, k], B[i, k], G[i, k], k)
    return out


def invalid_rays():
    base = rays_of([[5.0, 4.0, 2.5]] * len(INVALID_KINDS), [[0.3, -0.5, 0.2]] * len(INVALID_KINDS), 1e-4, 100.0)
    nan, inf = F(np.nan), F(np.inf)
    base[0, 1] = nan; base[1, 2] = -inf; base[2, 4] = nan; base[3, 6] = inf; base[4, 4:7] = (0.0, -0.0, 0.0)
    base[5, 3] = nan; base[6, 3] = -inf; base[7, 7] = nan; base[8, 7] = inf; base[9, 3], base[9, 7] = 2.0, 1.0
    return base


class Batch:
    """the mixed batch of one scene with the oracle's answers, computed once"""

    def __init__(self, sd, seed=11):
        rng = np.random.RandomState(seed)
        self.sd, self.osc = sd, oa.Scene(sd)
        V = self.V = sd.triangle_soup()[0]
        ntri = V.shape[0]
        self.light = (sd.light_first, sd.light_count)
        parts, kinds = [], []

        def add(kind, r):
            parts.append(r); kinds.extend([kind] * r.shape[0])

        def interior(n):
            tri = rng.randint(0, ntri, n)
            b = rng.uniform(0.1, 0.45, n).astype(F); g = rng.uniform(0.1, 0.45, n).astype(F)
            return on_triangle(V, tri, b, g)
        # origins in free space aimed at interior points of random triangles (t = 1 at the target)
        o = free_points(rng, 1502); aimed = rays_of(o, interior(1502) - o, 1e-4, 3.0e38)
        add("aimed", aimed)
        # uniform random directions with short far bounds: many misses
        add("random", rays_of(free_points(rng, 800), unit(rng, 800), 1e-4, rng.uniform(0.1, 6.0, 800).astype(F)))
        # axis-aligned directions: zero components, some of them negative zeros
        d = np.zeros((400, 3), F); d[np.arange(400), rng.randint(0, 3, 400)] = rng.choice([-1.0, 1.0, 2.5, -0.5], 400)
        d[rng.rand(400, 3) < 0.5] *= F(-1.0)          # (flips the sign of zeros too: -0.0)
        add("axis", rays_of(free_points(rng, 400), d, 1e-4, 3.0e38))
        # origins exactly on a surface (the faces are axis-aligned: the shared coordinate is exact), tmin = 0 and tmin = 1e-4
        for tmin in (0.0, 1e-4):
            tri = rng.randint(0, ntri, 300)
            p = on_triangle(V, tri, rng.uniform(0.1, 0.45, 300).astype(F), rng.uniform(0.1, 0.45, 300).astype(F))
            add(f"surface tmin {tmin:g}", rays_of(p, unit(rng, 300), tmin, 3.0e38))
        # rays aimed at shared edges (a point on the edge p0 p1 / p1 p2) and at vertices of the tessellated boxes and walls
        tri = rng.randint(0, ntri, 400); s = rng.uniform(0.0, 1.0, 400).astype(F)
        edge = on_triangle(V, tri[:200], s[:200], np.zeros(200, F))
        edge2 = on_triangle(V, tri[200:300], (F(1) - s[200:300]).astype(F), s[200:300])
        vert = V[tri[300:]].reshape(100, 3, 3)[np.arange(100), rng.randint(0, 3, 100)]
        o = free_points(rng, 400)
        add("edges and vertices", rays_of(o, np.concatenate([edge, edge2, vert]) - o, 1e-4, 3.0e38))
        # the strict inequality at the far bound: for known hits, tmax = the reference t, one ulp below it, one ulp above it
        ref = oracle_closest(self.osc, aimed[:4 * N_TMAX], 0)
        known = np.nonzero(ref["triangle"] >= 0)[0][:N_TMAX]
        assert len(known) == N_TMAX
        t = ref["t"][known]
        for name, far in (("tmax = t", t), ("tmax = t - ulp", np.nextafter(t, F(0))), ("tmax = t + ulp", np.nextafter(t, F(np.inf)))):
            r = aimed[known].copy(); r[:, 7] = far
            add(name, r)
        rays = np.concatenate(parts)
        assert rays.shape[0] == N_RAYS - len(INVALID_KINDS), rays.shape
        # one of each invalid kind, scattered through the batch
        at = np.array([137, 511, 1026, 1600, 2047, 2500, 3001, 3333, 3800, 4000])
        self.invalid = at
        keep = np.ones(N_RAYS, bool); keep[at] = False
        self.rays = np.zeros((N_RAYS, 8), F); self.rays[keep] = rays; self.rays[at] = invalid_rays()
        self.kinds = np.empty(N_RAYS, object); self.kinds[keep] = kinds; self.kinds[at] = INVALID_KINDS
        self.valid = keep
        # references
        v = self.rays[keep]
        self.closest = {}
        for filt in (0, 1, 2):
            e = np.zeros(N_RAYS, ref.dtype); e[keep] = oracle_closest(self.osc, v, filt); e["triangle"][at] = -2
            self.closest[filt] = e
        self.occluded = np.full(N_RAYS, 2, np.uint8); self.occluded[keep] = oracle_occluded(self.osc, v)
        tree = np.full(N_RAYS, 2, np.uint8); tree[keep] = oracle_occluded(self.osc, v, brute=False)
        self.aside_occluded = tree != self.occluded
        # the brute force on 256 valid rays drawn from the whole batch
        valid_idx = np.nonzero(keep)[0]
        self.subset = np.sort(rng.choice(valid_idx, N_BRUTE, replace=False))
        self.table = brute_table(self.osc, V, self.rays[self.subset])
        self.aside = {}
        for filt in (0, 1, 2):
            b = brute_closest(self.table, self.rays[self.subset], self.light, filt)
            a = np.zeros(N_RAYS, bool)
            a[self.subset] = np.array([x.tobytes() != y.tobytes() for x, y in zip(b, self.closest[filt][self.subset])])
            self.aside[filt] = a

    def check_closest(self, hits, filt, what):
        want, aside = self.closest[filt], self.aside[filt]
        assert hits.dtype.itemsize == 16 and hits.shape == (N_RAYS,)
        bad = [i for i in np.nonzero(~aside)[0] if hits[i].tobytes() != want[i].tobytes()]
        assert not bad, f"{what}: {len(bad)} rays differ from evo_closest, first {[(i, self.kinds[i], hits[i], want[i]) for i in bad[:4]]}"
        L = self.osc.lib
        t, b, g = C.c_float(), C.c_float(), C.c_float()
        for i in np.nonzero(aside)[0]:                      # (set aside: any triangle the test accepts with the reported t bits)
            k, r = int(hits["triangle"][i]), self.rays[i]
            if k < 0:
                continue
            c = [np.ascontiguousarray(self.V[k, j:j + 3]) for j in (0, 3, 6)]
            o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
            assert L.evo_tri_test(oa.ptr(c[0]), oa.ptr(c[1]), oa.ptr(c[2]), oa.ptr(o), oa.ptr(d), float(r[3]), float(r[7]), C.byref(t), C.byref(b), C.byref(g)), (what, i)
            assert F(t.value).tobytes() == hits["t"][i].tobytes(), (what, i)

    def check_occluded(self, out, what):
        assert out.dtype == np.uint8 and out.shape == (N_RAYS,)
        bad = np.nonzero((out != self.occluded) & ~self.aside_occluded)[0]
        assert len(bad) == 0, f"{what}: {len(bad)} rays differ from evo_occluded_brute, first {[(i, self.kinds[i], out[i], self.occluded[i]) for i in bad[:4]]}"


@pytest.fixture(scope="module")
def room():
    return scenes.box_room(seed=3, n_boxes=6, tess=2, aspect=W / H)


@pytest.fixture(scope="module")
def batch(oracle, room):
    b = Batch(room)
    for filt in (0, 1, 2):
        assert b.aside[filt].sum() == 0, "box_room: evo_closest and the brute force agree on all 256 rays"
    assert b.aside_occluded.sum() <= 0.005 * N_RAYS
    hit = b.closest[0]["triangle"] >= 0
    say(f"batch: {N_RAYS} rays, {int(hit.sum())} hit, {int((b.closest[0]['triangle'] == -1).sum())} miss, {len(b.invalid)} invalid; occluded {int((b.occluded == 1).sum())}; "
        f"set aside {int(b.aside[0].sum())} / {int(b.aside_occluded.sum())}; light-only hits {int((b.closest[2]['triangle'] >= 0).sum())}")
    # the batch exercises what it is meant to: hits and misses, the strict far bound, both sides of the light filter
    k = b.kinds
    assert hit[k == "tmax = t + ulp"].all() and not hit[k == "tmax = t"].any() and not hit[k == "tmax = t - ulp"].any()
    assert 0.2 < hit.mean() < 0.98 and (b.closest[2]["triangle"] >= 0).any() and (b.closest[1]["triangle"] != b.closest[0]["triangle"]).any()
    return b


def context(evplp, sd, builder=1):
    c = evplp.Context(W, H, NP, NP, P, bvh_builder=builder, deterministic=True)
    sd.upload(c)
    return c


@pytest.fixture(scope="module")
def sah_results(evplp, room, batch):
    """the SAH context's answers for the mixed batch: what the builders, the device form, the ordering pass and the group are compared with"""
    with context(evplp, room) as c:
        return {f: c.trace_closest(batch.rays, f) for f in (0, 1, 2)}, c.trace_occluded(batch.rays)


# ---- 1: against the references
def test_closest_hit_with_each_filter_and_occlusion_match_the_oracle(batch, sah_results):
    closest, occluded = sah_results
    for filt in (0, 1, 2):
        batch.check_closest(closest[filt], filt, f"filter {filt}")
        inv = closest[filt][batch.invalid]
        assert (inv["triangle"] == -2).all() and (inv["t"] == 0).all() and (inv["beta"] == 0).all() and (inv["gamma"] == 0).all(), inv
    batch.check_occluded(occluded, "occlusion")
    assert (occluded[batch.invalid] == 2).all() and (occluded[batch.valid] < 2).all()
    # an invalid ray's neighbours are untouched by it: they are in the comparison above, and they are valid rays with answers of their own
    for i in batch.invalid:
        for j in (i - 1, i + 1):
            assert batch.valid[j] and closest[0]["triangle"][j] >= -1 and closest[0][j].tobytes() == batch.closest[0][j].tobytes()
    # the strict inequality at the far bound
    k = batch.kinds
    assert (closest[0]["triangle"][k == "tmax = t + ulp"] >= 0).all()
    assert (closest[0]["triangle"][k == "tmax = t"] == -1).all(), "t < tmax is strict: tmax = t does not report that hit"
    assert (closest[0]["triangle"][k == "tmax = t - ulp"] == -1).all()


# ---- 2: builder independence
@pytest.mark.parametrize("builder", [0, 2, 3, 4])
def test_every_builder_gives_the_sah_trees_bytes(evplp, room, batch, sah_results, builder):
    closest, occluded = sah_results
    with context(evplp, room, builder) as c:
        assert c.accel_info()["builder"] == BUILDERS[builder]
        for filt in (0, 1, 2):
            got = c.trace_closest(batch.rays, filt)
            keep = ~batch.aside[filt]
            assert got[keep].tobytes() == closest[filt][keep].tobytes(), (BUILDERS[builder], filt, np.nonzero(got != closest[filt])[0][:8])
        got = c.trace_occluded(batch.rays)
        keep = ~batch.aside_occluded
        assert got[keep].tobytes() == occluded[keep].tobytes(), BUILDERS[builder]


# ---- 3: deep trees
def test_deep_chain_tree_fits_the_stack_and_equals_the_sah_tree(evplp):
    sd = scenes.morton_chain_full(aspect=W / H)
    eye, dirs = wr.primary_rays(sd, W, H, (0.003, -0.002))
    primary = rays_of(np.broadcast_to(eye, (W * H, 3)), dirs.reshape(-1, 3), 0.1, 100.0)
    xs, ys = np.meshgrid(np.linspace(-2.5, 2.5, 24, dtype=F), np.linspace(-2.5, 2.5, 24, dtype=F))
    o = np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, -1.5, F)], axis=1)
    along = np.concatenate([rays_of(o, [[0.0, 0.0, 1.0]] * len(o), 1e-4, 3.0e38), rays_of(o + F(0.001), [[0.01, -0.02, 1.0]] * len(o), 1e-4, 3.0e38)])
    rays = np.concatenate([primary, along])
    with context(evplp, sd, 0) as c:
        info = c.accel_info()
        assert info["builder"] == "lbvh" and 59 <= info["depth"] <= 62
        n4 = c.debug_accel(4)
        worst = wr.worst_case_entries(n4)
        generic = 3 * ((info["depth"] + 1) // 2) + 4
        allocated = min(info["stack4_entries"], generic) if info["stack4_entries"] > 0 else generic        # kernels.h lane_stack_bytes4
        sp = max(wr.replay_closest(n4, primary[:, 0:3], primary[:, 4:7], 0.1, 100.0).max(), wr.replay_closest(n4, along[:, 0:3], along[:, 4:7], 1e-4).max())
        say(f"deep tree: depth {info['depth']}, stack4_entries {info['stack4_entries']}, worst {worst}, allocated {allocated} entries ({allocated * 256} B of LDS per wave), replayed sp {int(sp)}")
        # before any launch: what these rays hold fits what the launcher allocates, and that fits a workgroup's LDS
        assert int(sp) <= worst <= allocated and allocated * 256 <= 64 * 1024
        assert int(sp) >= wr.LT_LDS_ENTRIES + 4, "the rays along the chain reach deeper than a balanced tree's stack"
        deep = c.trace_closest(rays), c.trace_occluded(rays)
    with context(evplp, sd, 1) as c:
        assert c.accel_info()["builder"] == "sah"
        sah = c.trace_closest(rays), c.trace_occluded(rays)
    assert deep[0].tobytes() == sah[0].tobytes(), np.nonzero(deep[0] != sah[0])[0][:8]
    assert deep[1].tobytes() == sah[1].tobytes()
    assert (sah[0]["triangle"] >= 0).mean() > 0.5 and (sah[1] == 1).any()


# ---- 4: chunk boundaries
def test_small_batches_are_prefixes_of_the_large_one(evplp, room, batch, sah_results):
    closest, occluded = sah_results
    with context(evplp, room) as c:
        for n in (1, 63, 64, 65):
            assert c.trace_closest(batch.rays[:n]).tobytes() == closest[0][:n].tobytes(), n
            assert c.trace_occluded(batch.rays[:n]).tobytes() == occluded[:n].tobytes(), n
        # n = 0 touches nothing
        L = evplp.lib()
        canary_h = np.full(4, 0x5A, np.uint8).repeat(16).view(evplp.HIT_DTYPE).copy(); canary_o = np.full(16, 0x5A, np.uint8)
        before = canary_h.tobytes(), canary_o.tobytes()
        assert L.evplp_trace_closest(c._h, batch.rays.ctypes.data, 0, 0, 0, canary_h.ctypes.data) == evplp.OK
        assert L.evplp_trace_occluded(c._h, batch.rays.ctypes.data, 0, 0, canary_o.ctypes.data) == evplp.OK
        assert L.evplp_trace_closest(c._h, None, 0, 0, 0, None) == evplp.OK and L.evplp_trace_occluded(c._h, None, 0, 0, None) == evplp.OK
        assert (canary_h.tobytes(), canary_o.tobytes()) == before
        assert len(c.trace_closest(np.zeros((0, 8), F))) == 0 and len(c.trace_occluded(np.zeros((0, 8), F))) == 0


def one_triangle_scene():
    s = scenes.SceneData()
    m = s.add_material((0.5, 0.5, 0.5)); lm = s.add_material((0, 0, 0))
    s.add_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], m)
    s.light_mesh = s.add_quad([0.0, 0.0, 3.0], [0, 0.5, 0], [0.5, 0, 0], lm)
    s.cam_origin = [0.3, 0.3, 2.0]; s.cam_lookat = [0.3, 0.3, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.triangle_soup()
    return s


def test_batches_across_the_chunk_boundary_equal_single_chunk_calls(evplp):
    Cn = evplp.QUERY_CHUNK_RAYS
    n = 2 * Cn + 3
    rays = np.zeros((n, 8), F)
    rays[:, 0:3] = (5.0, 5.0, 5.0); rays[:, 4:7] = (1.0, 2.0, 3.0); rays[:, 3] = 1e-4; rays[:, 7] = 10.0      # away from everything: cheap misses
    rays[:, 0] += (np.arange(n) % 1024).astype(F)
    for i in (0, Cn - 2, Cn - 1, Cn, Cn + 1, 2 * Cn - 1, 2 * Cn, 2 * Cn + 2):                                 # a hit on either side of every boundary
        rays[i] = (0.2, 0.2 + 0.1 * (i % 3), 1.0, 0.0, 0.0, 0.0, -1.0, 5.0)
    rays[Cn + 7, 4:7] = 0.0                                                                                   # and an invalid ray behind one
    with context(evplp, one_triangle_scene()) as c:
        parts = [(c.trace_closest(rays[a:b]), c.trace_occluded(rays[a:b])) for a, b in ((0, Cn), (Cn, 2 * Cn), (2 * Cn, n))]
        whole_c = np.concatenate([p[0] for p in parts]); whole_o = np.concatenate([p[1] for p in parts])
        assert (whole_c["triangle"] >= 0).sum() == 8 and (whole_o == 1).sum() == 8 and whole_c["triangle"][Cn + 7] == -2 and whole_o[Cn + 7] == 2
        for m in (Cn - 1, Cn, Cn + 1, n):
            assert c.trace_closest(rays[:m]).tobytes() == whole_c[:m].tobytes(), m
            assert c.trace_occluded(rays[:m]).tobytes() == whole_o[:m].tobytes(), m
        assert c.trace_closest(rays, order=True).tobytes() == whole_c.tobytes() and c.trace_occluded(rays, order=True).tobytes() == whole_o.tobytes()


# ---- 5: moving scenes
def test_a_moved_mesh_is_refused_until_the_refit_and_then_hit_where_it_is(evplp, oracle, room):
    mesh = 6 + 5                                    # the top face of the first box
    m = [1, 0, 0, 0.3, 0, 1, 0, 0.2, 0, 0, 1, 0.7]
    rng = np.random.RandomState(5)
    with context(evplp, room) as c:
        c.transform_mesh(mesh, m)
        for call in (lambda: c.trace_closest(np.zeros((1, 8), F)), lambda: c.trace_occluded(np.zeros((1, 8), F))):
            with pytest.raises(evplp.EvplpError) as e:
                call()
            assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value)
        c.refit_accel()
        moved = copy.deepcopy(room)
        for k in range(len(moved.meshes)):
            moved.meshes[k]["verts"] = c.mesh_vertices(k, 0)
        assert not np.array_equal(moved.meshes[mesh]["verts"], room.meshes[mesh]["verts"])
        V = moved.triangle_soup()[0]
        first = sum(len(mm["idx"]) for mm in moved.meshes[:mesh]); count = len(moved.meshes[mesh]["idx"])
        # rays from above aimed at the moved face, and random ones through the room
        tri = first + rng.randint(0, count, 256)
        target = on_triangle(V, tri, rng.uniform(0.1, 0.45, 256).astype(F), rng.uniform(0.1, 0.45, 256).astype(F))
        o = (target + np.array([0.0, 0.0, 1.0], F) + rng.uniform(-0.2, 0.2, (256, 3))).astype(F)
        rays = np.concatenate([rays_of(o, target - o, 1e-4, 3.0e38), rays_of(free_points(rng, 256), unit(rng, 256), 1e-4, 3.0e38)])
        osc = oa.Scene(moved)
        want, want_o = oracle_closest(osc, rays, 0), oracle_occluded(osc, rays)
        got, got_o = c.trace_closest(rays), c.trace_occluded(rays)
        assert got.tobytes() == want.tobytes(), np.nonzero(got != want)[0][:8]
        assert got_o.tobytes() == want_o.tobytes()
        on_moved = (want["triangle"][:256] >= first) & (want["triangle"][:256] < first + count)
        assert on_moved.sum() > 64, "rays aimed at the moved face reach it"
        for i in np.nonzero(on_moved)[0][:32]:
            assert c.triangle_info(got["triangle"][i]) == (mesh, int(got["triangle"][i]) - first)
        assert c.triangle_info(0) == (0, 0) and c.triangle_info(V.shape[0] - 1)[0] == len(moved.meshes) - 1
        for bad in (-1, V.shape[0]):
            with pytest.raises(evplp.EvplpError):
                c.triangle_info(bad)
        # the same rays on the scene as it was built hit elsewhere: the query follows the refit
        with context(evplp, room) as c0:
            assert c0.trace_closest(rays).tobytes() != got.tobytes()


# ---- 6: the device form
def test_a_device_tensor_gives_the_host_forms_bytes_and_calls_need_no_wait_between_them(evplp, room, batch, sah_results):
    import torch
    closest, occluded = sah_results
    with context(evplp, room) as c:
        d = torch.from_numpy(batch.rays).cuda()
        torch.cuda.synchronize()
        h1 = c.trace_closest(d, 1)
        h0 = c.trace_closest(d)               # enqueued behind the first without a wait in between
        o0 = c.trace_occluded(d)
        h0b = c.trace_closest(d, order=True)
        c.synchronize()
        assert isinstance(h0, torch.Tensor) and h0.is_cuda and h0.dtype == torch.int32 and tuple(h0.shape) == (N_RAYS, 4) and o0.dtype == torch.uint8
        as_hits = lambda t: t.cpu().numpy().view(evplp.HIT_DTYPE).reshape(-1)      # noqa: E731
        assert as_hits(h0).tobytes() == closest[0].tobytes() and as_hits(h1).tobytes() == closest[1].tobytes()
        assert as_hits(h0b).tobytes() == closest[0].tobytes()
        assert o0.cpu().numpy().tobytes() == occluded.tobytes()


# ---- 7: the ordering pass
def test_the_ordering_pass_changes_no_byte(evplp, room, batch, sah_results):
    closest, occluded = sah_results
    rng = np.random.RandomState(9)
    d = np.abs(unit(rng, 1000)) + F(0.01)
    one_key = rays_of([[4.0, 3.0, 2.0]] * 1000, d, 1e-4, 3.0e38)             # one origin, one octant: every ray has the same key
    with context(evplp, room) as c:
        for filt in (0, 1, 2):
            assert c.trace_closest(batch.rays, filt, order=True).tobytes() == closest[filt].tobytes(), filt
        assert c.trace_occluded(batch.rays, order=True).tobytes() == occluded.tobytes()
        plain = c.trace_closest(one_key), c.trace_occluded(one_key)
        assert (plain[0]["triangle"] >= 0).all()
        assert c.trace_closest(one_key, order=True).tobytes() == plain[0].tobytes() and c.trace_occluded(one_key, order=True).tobytes() == plain[1].tobytes()


# ---- 9: refusals
def test_refusals_leave_the_context_usable_and_write_nothing(evplp, room, batch, sah_results):
    L = evplp.lib()
    rays = batch.rays[:8].copy()
    hits = np.full(8 * 16, 0x5A, np.uint8); out = np.full(8, 0x5A, np.uint8)
    rp, hp, op = rays.ctypes.data, hits.ctypes.data, out.ctypes.data
    with evplp.Context(W, H, NP, NP, P) as c:                   # no evplp_build_accel yet
        assert L.evplp_trace_closest(c._h, rp, 8, 0, 0, hp) == evplp.ERR_INVALID and b"evplp_build_accel" in L.evplp_last_error(c._h)
        assert L.evplp_trace_occluded(c._h, rp, 8, 0, op) == evplp.ERR_INVALID
        assert L.evplp_trace_closest_device(c._h, rp, 8, 0, 0, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_occluded_device(c._h, rp, 8, 0, op) == evplp.ERR_INVALID
        assert L.evplp_triangle_info(c._h, 0, None, None) == evplp.ERR_INVALID
        room.upload(c)
        assert L.evplp_trace_closest(c._h, rp, -1, 0, 0, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_occluded(c._h, rp, -1, 0, op) == evplp.ERR_INVALID
        assert L.evplp_trace_closest(c._h, None, 8, 0, 0, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_closest(c._h, rp, 8, 0, 0, None) == evplp.ERR_INVALID
        assert L.evplp_trace_occluded(c._h, None, 8, 0, op) == evplp.ERR_INVALID
        assert L.evplp_trace_occluded(c._h, rp, 8, 0, None) == evplp.ERR_INVALID
        assert L.evplp_trace_closest(c._h, rp, 8, 3, 0, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_closest(c._h, rp, 8, -1, 0, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_closest(c._h, rp, 8, 0, 2, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_occluded(c._h, rp, 8, 4, op) == evplp.ERR_INVALID
        assert L.evplp_trace_closest_device(c._h, None, 8, 0, 0, hp) == evplp.ERR_INVALID
        assert L.evplp_trace_occluded_device(c._h, rp, 8, 8, op) == evplp.ERR_INVALID
        assert (hits == 0x5A).all() and (out == 0x5A).all(), "a refused call writes nothing"
        assert c.trace_closest(rays).tobytes() == sah_results[0][0][:8].tobytes() and c.trace_occluded(rays).tobytes() == sah_results[1][:8].tobytes()
