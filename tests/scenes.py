"""Seeded test scenes shared by the oracle and the HIP path (inputs only -- no rendering here)."""
import math
import os

import numpy as np


class SceneData:
    def __init__(self):
        self.meshes = []      # dict(verts (n,3) f32, uvs (n,2) f32, idx (m,3) i32, material int)
        self.materials = []   # dict(kd, ks, ns, tex_kd, tex_ks, tex_ns)
        self.textures = []    # (h, w, 4) float32
        self.light_mesh = -1
        self.light_intensity = [17.0, 12.0, 4.0, 0.0]
        self.cam_origin = [0.0, 0.0, 0.0]
        self.cam_lookat = [0.0, 1.0, 0.0]
        self.cam_up = [0.0, 0.0, 1.0]
        self.fovy = math.radians(60.0)
        self.aspect = 1.0

    # ---- construction helpers
    def add_material(self, kd, ks=(0, 0, 0), ns=0.0, tex_kd=-1, tex_ks=-1, tex_ns=-1):
        self.materials.append(dict(kd=[float(x) for x in kd], ks=[float(x) for x in ks], ns=float(ns),
                                   tex_kd=tex_kd, tex_ks=tex_ks, tex_ns=tex_ns))
        return len(self.materials) - 1

    def add_mesh(self, verts, idx, material, uvs=None):
        verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1, 3)
        uvs = np.zeros((verts.shape[0], 2), np.float32) if uvs is None else np.ascontiguousarray(uvs, dtype=np.float32).reshape(-1, 2)
        self.meshes.append(dict(verts=verts, uvs=uvs, idx=idx, material=material))
        return len(self.meshes) - 1

    def add_quad(self, o, u, v, material, nu=1, nv=1):
        """Tessellated parallelogram with normal along u x v."""
        o, u, v = (np.asarray(a, dtype=np.float32) for a in (o, u, v))
        s, t = np.meshgrid(np.arange(nu + 1, dtype=np.float32) / nu, np.arange(nv + 1, dtype=np.float32) / nv)
        verts = o[None, None, :] + s[..., None] * u[None, None, :] + t[..., None] * v[None, None, :]
        uvs = np.stack([s, t], axis=-1)
        idx = []
        for j in range(nv):
            for i in range(nu):
                a = j * (nu + 1) + i; b = a + 1; c = b + nu + 1; d = a + nu + 1
                idx += [(a, b, c), (a, c, d)]
        return self.add_mesh(verts.reshape(-1, 3), idx, material, uvs.reshape(-1, 2))

    def add_box(self, lo, hi, material, outward=True, n=1):
        lo = np.asarray(lo, np.float32); hi = np.asarray(hi, np.float32); d = hi - lo
        ids = []
        for axis in range(3):
            for side in range(2):
                a1, a2 = (axis + 1) % 3, (axis + 2) % 3
                o = lo.copy(); u = np.zeros(3, np.float32); v = np.zeros(3, np.float32)
                if side:
                    o[axis] = hi[axis]
                if (side == 1) == outward:
                    u[a1] = d[a1]; v[a2] = d[a2]
                else:
                    u[a2] = d[a2]; v[a1] = d[a1]
                ids.append(self.add_quad(o, u, v, material, n, n))
        return ids

    def merge_meshes(self, ids, material):
        """Concatenate several meshes into one (e.g. the single light mesh)."""
        verts, uvs, idx, base = [], [], [], 0
        for i in ids:
            m = self.meshes[i]
            verts.append(m["verts"]); uvs.append(m["uvs"]); idx.append(m["idx"] + base); base += m["verts"].shape[0]
        keep = [m for k, m in enumerate(self.meshes) if k not in ids]
        self.meshes = keep
        return self.add_mesh(np.concatenate(verts), np.concatenate(idx), material, np.concatenate(uvs))

    # ---- views
    def triangle_soup(self):
        """Flattened (verts9, uv6, material) in mesh order, the light mesh keeps its place."""
        V, U, M = [], [], []
        first = 0
        for k, m in enumerate(self.meshes):
            v = m["verts"][m["idx"]].reshape(-1, 9); u = m["uvs"][m["idx"]].reshape(-1, 6)
            if k == self.light_mesh:
                self.light_first, self.light_count = first, v.shape[0]
            V.append(v); U.append(u); M.append(np.full(v.shape[0], m["material"], np.int32)); first += v.shape[0]
        return (np.ascontiguousarray(np.concatenate(V), np.float32), np.ascontiguousarray(np.concatenate(U), np.float32),
                np.ascontiguousarray(np.concatenate(M), np.int32))

    def upload(self, ctx):
        """Feed an evplp_amd.Context through the C ABI (textures, materials, meshes, light, camera, accel)."""
        tex_ids = [ctx.add_texture(t) for t in self.textures]
        mat_ids = []
        for m in self.materials:
            mat_ids.append(ctx.add_material(m["kd"], m["ks"], m["ns"],
                                            tex_ids[m["tex_kd"]] if m["tex_kd"] >= 0 else -1,
                                            tex_ids[m["tex_ks"]] if m["tex_ks"] >= 0 else -1,
                                            tex_ids[m["tex_ns"]] if m["tex_ns"] >= 0 else -1))
        light = -1
        for k, m in enumerate(self.meshes):
            mid = ctx.add_mesh(m["verts"], m["idx"], mat_ids[m["material"]], m["uvs"])
            if k == self.light_mesh:
                light = mid
        ctx.set_arealight(light, self.light_intensity)
        ctx.set_camera(self.cam_origin, self.cam_lookat, self.cam_up, self.fovy, self.aspect)
        ctx.build_accel()


def box_room(seed=1, n_boxes=6, tess=2, glossy=True, textured=False, aspect=1.0):
    """Closed room [0,10]x[0,8]x[0,5] with random boxes, one ceiling light (2 quads merged), a camera inside."""
    rng = np.random.RandomState(seed)
    s = SceneData()
    s.aspect = aspect
    tex = -1
    if textured:
        t = np.zeros((8, 8, 4), np.float32)
        t[..., :3] = 0.25 + 0.5 * rng.rand(8, 8, 3).astype(np.float32)
        s.textures.append(t)
        tex = 0
    wall = [s.add_material(0.2 + 0.6 * rng.rand(3)) for _ in range(5)]
    floor = s.add_material(0.2 + 0.6 * rng.rand(3), tex_kd=tex)
    mats = wall + [floor]
    # room shell, normals inward: one material per face
    lo, hi = np.array([0, 0, 0], np.float32), np.array([10, 8, 5], np.float32)
    d = hi - lo
    k = 0
    for axis in range(3):
        for side in range(2):
            a1, a2 = (axis + 1) % 3, (axis + 2) % 3
            o = lo.copy(); u = np.zeros(3, np.float32); v = np.zeros(3, np.float32)
            if side:
                o[axis] = hi[axis]
            if side == 0:
                u[a1] = d[a1]; v[a2] = d[a2]
            else:
                u[a2] = d[a2]; v[a1] = d[a1]
            m = mats[5] if (axis == 2 and side == 0) else mats[k % 5]
            s.add_quad(o, u, v, m, tess * 2, tess * 2)
            k += 1
    for b in range(n_boxes):
        c = np.array([1.5 + 7.0 * rng.rand(), 1.5 + 5.0 * rng.rand(), 0.0])
        sz = np.array([0.4 + 1.2 * rng.rand(), 0.4 + 1.2 * rng.rand(), 0.5 + 2.5 * rng.rand()])
        ks = (0.2, 0.2, 0.2) if (glossy and b % 3 == 2) else (0, 0, 0)
        ns = 20.0 if (glossy and b % 3 == 2) else 0.0
        m = s.add_material(0.2 + 0.6 * rng.rand(3), ks, ns)
        s.add_box(c - [sz[0] / 2, sz[1] / 2, 0], c + [sz[0] / 2, sz[1] / 2, sz[2]], m, True, tess)
    # light: two quads facing down, merged into one mesh
    lm = s.add_material((0, 0, 0))
    a = s.add_quad([3.0, 3.0, 4.9], [0, 1.5, 0], [1.5, 0, 0], lm, 2, 2)
    b = s.add_quad([6.0, 3.5, 4.9], [0, 1.0, 0], [2.0, 0, 0], lm, 1, 1)
    s.light_mesh = s.merge_meshes([a, b], lm)
    s.light_intensity = [17.0, 12.0, 4.0, 0.0]
    s.cam_origin = [9.2, 0.9, 3.2]; s.cam_lookat = [3.0, 5.0, 2.9]; s.cam_up = [0.0, 0.0, 1.0]
    s.fovy = math.radians(55.0)
    s.triangle_soup()
    return s


def _chain_stage(s, aspect):
    """What the two Morton-chain scenes share.  A floor at z = -2 and a small anchor triangle at z = 2 fix the box of the triangles' box
    centres, which the LBVH builders quantise, to [0, 1] x [0, 1] x [-2, 2]; the light (a quad at z = -1 facing +z, box centre inside that
    box) and the camera sit below the sheets, which are added next in the planes 0 <= z <= 1.  A light path's first segment and every
    primary ray therefore cross the whole chain along +z.  Returns the sheets' material (diffuse plus glossy)."""
    s.aspect = aspect
    sheet = s.add_material((0.55, 0.5, 0.45), (0.25, 0.25, 0.25), 12.0)
    ground = s.add_material((0.6, 0.6, 0.6))
    lm = s.add_material((0, 0, 0))
    s.add_quad([-4.5, -4.5, -2.0], [9.0, 0, 0], [0, 9.0, 0], ground)                                 # box centre (0, 0, -2), faces +z
    s.add_mesh([[0.9, 0.9, 2.0], [1.0, 1.1, 2.0], [1.1, 0.9, 2.0]], [[0, 1, 2]], ground)             # box centre (1, 1, 2), faces -z
    s.light_mesh = s.add_quad([0.3, 0.3, -1.0], [0.4, 0, 0], [0, 0.4, 0], lm)
    s.light_intensity = [17.0, 12.0, 4.0, 4.0]                 # (an emission lobe of exponent 4 around +z)
    s.cam_origin = [1.1, 0.2, -1.5]; s.cam_lookat = [0.3, 0.5, 1.0]; s.cam_up = [0.05, 1.0, 0.0]
    s.fovy = math.radians(50.0)
    return sheet


def _sheet(cx, cy, hx, hy, z):
    """One triangle in the plane z whose box is [cx - hx, cx + hx] x [cy - hy, cy + hy], facing -z (towards the light and the camera: light
    tracing ends a path on a back face)"""
    return [[cx + hx, cy - hy, z], [cx - hx, cy - hy, z], [cx, cy + hy, z]]


def morton_chain(levels=21, per=5, aspect=1.0):
    """Scene A: `levels` groups of `per` wide triangles whose box centres halve their distance to the origin from group to group
    (cx = 2^-L (1 + 0.05 j / per), z = cx / 2): clustered Morton codes, so the LBVH builders make a tree that is a chain of about one level
    per group where SAH makes a balanced one.  The sheets overlap almost completely as seen along z."""
    s = SceneData()
    mat = _chain_stage(s, aspect)
    tris = []
    for L in range(levels):
        for j in range(per):
            cx = 2.0 ** -L * (1.0 + 0.05 * j / per)
            tris += _sheet(cx, 0.0, 3.0, 3.0, 0.5 * cx)
    s.sheet_mesh = s.add_mesh(tris, np.arange(len(tris)).reshape(-1, 3), mat)
    s.triangle_soup()
    return s


def morton_chain_full(clusters=58, per=5, aspect=1.0):
    """Scene B: cluster k's Morton code has the single bit 62 - k set (beside the top z bit, which every sheet shares because the sheets
    lie in the upper half of the z range the floor opens): the radix tree over the sorted codes is one chain with a level per cluster, up
    to the 62 levels the builders accept.  bit % 3 = 2, 1, 0 puts the box centre on the x, y, z axis at 2^(bit / 3 - 21) of the range
    (times 1.0000001, rounded up to a multiple of 2^-22 so that centre -+ half-size is exact in fp32); the cluster's `per` triangles share
    that box centre exactly, with half-sizes 3 + 0.01 j.  Many triangles are coplanar and overlap: a closest hit there is decided by the
    lowest original index alone."""
    s = SceneData()
    mat = _chain_stage(s, aspect)
    tris = []
    for k in range(clusters):
        bit = 62 - k
        axis = 2 - bit % 3
        c = [0.0, 0.0, 0.0]
        if not (axis == 2 and bit // 3 == 20):            # (z's top bit is the shared one: that cluster keeps the plain code)
            v = float(np.float32(2.0 ** (bit // 3 - 21) * 1.0000001))
            c[axis] = math.ceil(v * 2.0 ** 22) / 2.0 ** 22 * (4.0 if axis == 2 else 1.0)
        for j in range(per):
            h = float(np.float32(3.0 + 0.01 * j))
            tris += _sheet(c[0], c[1], h, h, c[2])
    s.sheet_mesh = s.add_mesh(tris, np.arange(len(tris)).reshape(-1, 3), mat)
    s.triangle_soup()
    return s


def _rand_unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def oblique_soup(seed=1, aspect=1.0):
    """Random oblique triangles in [0, 10]^3 (sizes log-uniform 1e-3 .. 3, random orientation, three meshes of 180) and a mesh of planted
    ones, in this order (s.planted names their scene triangle indices):
      slivers       12 triangles of aspect 1e4 (long edge 1 .. 4, height 1e-4 of it)
      tiny          8 triangles whose edges are one or two ulps of their coordinates: area barely above zero in fp32
      no_area       8 triangles without area (a repeated corner, or three corners on a line with an exactly zero cross product): they are in
                    no tree and no query may report them
      ties          two pairs of triangles with identical corners, (a, b) and (c, d) with a < b, c < d and other triangles in between
      coplanar      two overlapping triangles in the plane x + y + z = 15 (small integer corners: exactly coplanar)
      fan           8 triangles around the shared corner s.fan_hub
    The light is a quad under the top of the cube, facing down; the camera looks at the cube's centre from outside."""
    rng = np.random.RandomState(seed)
    s = SceneData()
    s.aspect = aspect
    mats = [s.add_material(0.2 + 0.6 * rng.rand(3)) for _ in range(4)]
    for m in range(3):
        n = 180
        c = rng.uniform(0.5, 9.5, size=(n, 3))
        size = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), n))
        u, w = _rand_unit(rng, n), _rand_unit(rng, n)
        tri = np.stack([c - size[:, None] * (u + w) / 3.0, c + size[:, None] * (2.0 * u - w) / 3.0, c + size[:, None] * (2.0 * w - u) / 3.0], axis=1)
        s.add_mesh(np.clip(tri, 0.0, 10.0).reshape(-1, 3), np.arange(3 * n).reshape(-1, 3), mats[m])
    tris, names = [], {}

    def plant(name, t):
        names.setdefault(name, []).extend(range(len(tris), len(tris) + len(t)))
        tris.extend(t)
    sl = []
    for _ in range(12):
        p = rng.uniform(2.0, 8.0, 3); u, w = _rand_unit(rng, 1)[0], _rand_unit(rng, 1)[0]
        w = w - u * (u @ w); w /= np.linalg.norm(w)
        L = rng.uniform(1.0, 4.0)
        sl.append([p - 0.5 * L * u, p + 0.5 * L * u, p + rng.uniform(-0.4, 0.4) * L * u + 1e-4 * L * w])
    plant("slivers", np.clip(np.array(sl), 0.0, 10.0))
    tiny = []
    for k in range(8):
        p = rng.uniform(1.0, 9.0, 3).astype(np.float32)
        a, b = p.copy(), p.copy()
        up = np.float32(np.inf)
        a[k % 3] = np.nextafter(np.nextafter(p[k % 3], up), up) if k & 1 else np.nextafter(p[k % 3], up)
        b[(k + 1) % 3] = np.nextafter(p[(k + 1) % 3], up)
        tiny.append([p, a, b])
    plant("tiny", np.array(tiny, np.float64))
    flat = []
    for k in range(4):
        p, q = rng.uniform(1.0, 9.0, 3), rng.uniform(1.0, 9.0, 3)
        flat.append([p, q, q] if k & 1 else [p, p, q])
    for k in range(4):
        p = np.round(rng.uniform(1.0, 5.0, 3) * 4.0) / 4.0; e = np.array([1.0, 0.5, 0.25])[[k % 3, (k + 1) % 3, (k + 2) % 3]]
        flat.append([p, p + e, p + 3.0 * e])                      # (quarters: the edges and their cross product are exact, and zero)
    plant("no_area", np.array(flat))
    ta = np.array([[2.0, 2.5, 3.0], [4.5, 2.0, 6.0], [2.5, 5.0, 4.0]]); tb = np.array([[7.0, 6.5, 2.0], [5.5, 8.5, 4.5], [8.0, 8.0, 5.5]])
    plant("ties", [ta, tb])
    plant("coplanar", [np.array([[5.0, 5.0, 5.0], [8.0, 4.0, 3.0], [3.0, 8.0, 4.0]]), np.array([[6.0, 5.0, 4.0], [4.0, 7.0, 4.0], [7.0, 3.0, 5.0]])])
    hub = np.array([3.0, 6.5, 7.0]); ax = np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    e1 = np.cross(ax, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1); e2 = np.cross(ax, e1)
    rim = [hub + 0.4 * ax + 1.2 * (math.cos(a) * e1 + math.sin(a) * e2) for a in np.arange(8) * (math.pi / 4.0)]
    rim = np.array(rim, np.float32).astype(np.float64)
    plant("fan", [np.array([hub, rim[k], rim[(k + 1) % 8]]) for k in range(8)])
    plant("ties", [ta, tb])                                        # the second copy of each pair, behind everything planted since
    first = sum(len(m["idx"]) for m in s.meshes)
    s.add_mesh(np.array(tris).reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3), mats[3])
    s.planted = {k: [first + i for i in v] for k, v in names.items()}
    t = s.planted["ties"]
    s.planted["ties"] = [(t[0], t[2]), (t[1], t[3])]
    s.fan_hub = hub.astype(np.float32)
    lm = s.add_material((0, 0, 0))
    s.light_mesh = s.add_quad([4.0, 4.0, 9.9], [0, 2.0, 0], [2.0, 0, 0], lm)
    s.cam_origin = [22.0, -9.0, 12.0]; s.cam_lookat = [5.0, 5.0, 5.0]; s.cam_up = [0.0, 0.0, 1.0]
    s.fovy = math.radians(40.0)
    s.triangle_soup()
    return s


def flat_scene(seed=1, aspect=1.0):
    """Every triangle but the light's in the plane z = 0: an 8 x 8 tessellated quad over [0, 10] x [0, 8] and 200 random in-plane triangles
    over it, so no leaf box has any thickness.  The light quad sits above."""
    rng = np.random.RandomState(seed)
    s = SceneData()
    s.aspect = aspect
    s.add_quad([0.0, 0.0, 0.0], [10.0, 0, 0], [0, 8.0, 0], s.add_material((0.6, 0.6, 0.6)), 8, 8)
    n = 200
    c = np.concatenate([rng.uniform([0.5, 0.5], [9.5, 7.5], size=(n, 2)), np.zeros((n, 1))], axis=1)
    size = np.exp(rng.uniform(np.log(1e-2), np.log(3.0), n))
    ang = rng.uniform(0.0, 2.0 * math.pi, (n, 2))
    u = np.stack([np.cos(ang[:, 0]), np.sin(ang[:, 0]), np.zeros(n)], axis=1); w = np.stack([np.cos(ang[:, 1]), np.sin(ang[:, 1]), np.zeros(n)], axis=1)
    tri = np.stack([c - size[:, None] * (u + w) / 3.0, c + size[:, None] * (2.0 * u - w) / 3.0, c + size[:, None] * (2.0 * w - u) / 3.0], axis=1)
    s.add_mesh(tri.reshape(-1, 3), np.arange(3 * n).reshape(-1, 3), s.add_material((0.4, 0.5, 0.3)))
    lm = s.add_material((0, 0, 0))
    s.light_mesh = s.add_quad([4.0, 3.0, 3.0], [0, 2.0, 0], [2.0, 0, 0], lm)
    s.cam_origin = [5.0, -6.0, 6.0]; s.cam_lookat = [5.0, 4.0, 0.0]; s.cam_up = [0.0, 0.0, 1.0]
    s.fovy = math.radians(50.0)
    s.triangle_soup()
    return s


def moved(sd, scale=1.0, offset=(0.0, 0.0, 0.0)):
    """A copy of the scene with every vertex scaled about the origin and then translated, rounded to fp32 after the move; the camera
    goes with it.  Attributes a generator added (planted, fan_hub) are kept, the hub moved likewise."""
    import copy
    s = copy.deepcopy(sd)
    off = np.asarray(offset, np.float64)
    f = lambda p: (np.asarray(p, np.float64) * scale + off).astype(np.float32)       # noqa: E731
    for m in s.meshes:
        m["verts"] = np.ascontiguousarray(f(m["verts"]))
    s.cam_origin = [float(x) for x in f(s.cam_origin)]; s.cam_lookat = [float(x) for x in f(s.cam_lookat)]
    if hasattr(s, "fan_hub"):
        s.fan_hub = f(s.fan_hub)
    s.triangle_soup()
    return s


def load_obj_scene(json_path, decode=None):
    """Independent Python reading of a scene JSON + OBJ/MTL (same semantics as csrc/host/scene_io.cpp).
    decode(path) -> uint8 (h, w, 3) top-down pixels for map_Kd / map_Ks / map_Ns (RtTexture(filepath, 1.0),
    rtcommon.h:139-194: byte / 255, flipped vertically)."""
    import json
    root = json.load(open(json_path))
    d = os.path.dirname(json_path)
    s = SceneData()

    def read_mtl(path):
        out, cur = {}, None
        if not os.path.exists(path):
            return out
        for line in open(path):
            t = line.split()
            if not t:
                continue
            if t[0] == "newmtl":
                cur = t[1]; out[cur] = dict(kd=[0.6, 0.6, 0.6], ks=[0, 0, 0], ns=0.0)
            elif cur and t[0] == "Kd":
                out[cur]["kd"] = [float(x) for x in t[1:4]]
            elif cur and t[0] == "Ks":
                out[cur]["ks"] = [float(x) for x in t[1:4]]
            elif cur and t[0] == "Ns":
                out[cur]["ns"] = float(t[1])
            elif cur and t[0] in ("map_Kd", "map_Ks", "map_Ns"):
                out[cur][t[0]] = os.path.join(os.path.dirname(path), t[1])
        return out

    tex_ids = {}

    def tex_of(m, key):
        if key not in m:
            return -1
        if m[key] not in tex_ids:
            px = decode(m[key])
            t = np.zeros(px.shape[:2] + (4,), np.float32)
            t[..., :3] = px[::-1].astype(np.float32) / np.float32(255.0)
            tex_ids[m[key]] = len(s.textures); s.textures.append(t)
        return tex_ids[m[key]]

    def read_obj(path, want_materials):
        pos, tex, mtl = [], [], {}
        names, groups = [""], [dict(verts=[], uvs=[], idx=[], map={})]
        cur = 0
        for line in open(path):
            if line.startswith("v "):
                pos.append([np.float32(x) for x in line.split()[1:4]])
            elif line.startswith("vt"):
                tex.append([np.float32(x) for x in line.split()[1:3]])
            elif line.startswith("f "):
                face = []
                for tok in line.split()[1:]:
                    p = tok.split("/")
                    vi = int(p[0]); ti = int(p[1]) if len(p) > 1 and p[1] else 0
                    vi = vi - 1 if vi > 0 else len(pos) + vi
                    ti = (ti - 1 if ti > 0 else len(tex) + ti) if ti != 0 else -1
                    face.append((vi, ti))
                g = groups[cur]

                def idx_of(k):
                    if k not in g["map"]:
                        g["map"][k] = len(g["verts"])
                        g["verts"].append(pos[k[0]]); g["uvs"].append(tex[k[1]] if k[1] >= 0 else [0.0, 0.0])
                    return g["map"][k]
                for k in range(1, len(face) - 1):
                    g["idx"].append([idx_of(face[0]), idx_of(face[k]), idx_of(face[k + 1])])
            elif line.startswith("usemtl"):
                name = line.split()[1]
                if name not in names:
                    names.append(name); groups.append(dict(verts=[], uvs=[], idx=[], map={}))
                cur = names.index(name)
            elif line.startswith("mtllib"):
                mtl.update(read_mtl(os.path.join(os.path.dirname(path), line.split()[1])))
        res = []
        for name, g in zip(names, groups):
            if not g["idx"]:
                continue
            m = mtl.get(name, dict(kd=[0.6, 0.6, 0.6], ks=[0, 0, 0], ns=0.0))
            res.append((g, m))
        return res

    for rel in root["scene"]:
        for g, m in read_obj(os.path.join(d, rel), True):
            mid = s.add_material(m["kd"], m["ks"], m["ns"], tex_of(m, "map_Kd"), tex_of(m, "map_Ks"), tex_of(m, "map_Ns"))
            s.add_mesh(np.array(g["verts"], np.float32), np.array(g["idx"], np.int32), mid, np.array(g["uvs"], np.float32))
    lg = read_obj(os.path.join(d, root["arealight"]["obj"]), False)
    assert len(lg) == 1
    lm = s.add_material((0, 0, 0))
    s.light_mesh = s.add_mesh(np.array(lg[0][0]["verts"], np.float32), np.array(lg[0][0]["idx"], np.int32), lm, np.array(lg[0][0]["uvs"], np.float32))
    s.light_intensity = [float(x) for x in root["arealight"]["intensity"]]
    cam = root.get("camera", root.get("stablecamera"))
    s.aspect = float(np.float32(root["resX"]) / np.float32(root["resY"]))
    s.cam_origin, s.cam_lookat, s.cam_up = cam["origin"], cam["direction"], cam["up"]
    deg = np.float32(0.01745329251994329576923690768489)
    if "fovy" in cam:
        s.fovy = float(np.float32(cam["fovy"]) * deg)
    else:
        s.fovy = float(np.float32(2.0) * np.arctan2(np.tan(np.float32(cam["fovx"]) * deg * np.float32(0.5)), np.float32(s.aspect)))
    s.triangle_soup()
    return s, root
