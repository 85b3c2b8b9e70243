"""No GPU: the lightmap section's ABI surface, and the host twin of the atlas rasteriser (evplp_lightmap_cover: lightmap_raster.h, the header
the kernels of kernels_lightmap.hip include, compiled for the host) against the int64 restatement of tests/lightmap_restate.py -- inside or
not, and the bits of beta and gamma -- on triangles chosen to sit on the rules' edges: vertices exactly on sample centres, edges through
sample centres in all eight directions, both windings, slivers that cover no centre, UVs outside [0, 1], 8192-wide atlases, and UVs that do
not snap.  Then the property the ownership rule exists for: over a mesh whose vertices all lie on sample centres, every sample strictly
inside the union is covered by exactly one triangle and no sample by two."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lightmap_restate as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("evplp_surface_points", "evplp_surface_points_device", "evplp_lightmap_samples", "evplp_lightmap_samples_device", "evplp_lightmap_cover",
         "evplp_bake_lightmap", "evplp_bake_lightmap_device")
DIRS8 = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))


def test_symbols_are_exported_and_declared_and_the_abi_stays_5(evplp):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evplp.h")).read(), flags=re.S)
    lib = C.CDLL(evplp.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in evplp._SIGNATURES, name
    assert lib.evplp_abi_version() == 5 == evplp.ABI_VERSION
    assert evplp.LIGHTMAP_TEXEL_DTYPE.itemsize == 32 and C.sizeof(evplp.LightmapParams) == 24
    for method in ("surface_points", "surface_points_device", "lightmap_samples", "lightmap_samples_device", "bake_lightmap", "bake_lightmap_device"):
        assert hasattr(evplp.Context, method), method


def test_the_lightmap_structs_have_the_headers_layout(evplp, tmp_path):
    src = tmp_path / "lightmap_layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "evplp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %u %u %d\\n", sizeof(evplp_lightmap_params), sizeof(evplp_lightmap_texel), offsetof(evplp_lightmap_params, gutter),
           offsetof(evplp_lightmap_params, flags), offsetof(evplp_lightmap_texel, coverage), offsetof(evplp_lightmap_texel, photons),
           EVPLP_POINTS_WHITE, EVPLP_POINTS_FACE_EYES, EVPLP_LIGHTMAP_CHUNK);
    return 0;
}
''')
    exe = tmp_path / "lightmap_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [24, 32, 16, 20, 12, 28, evplp.POINTS_WHITE, evplp.POINTS_FACE_EYES, evplp.LIGHTMAP_CHUNK] == [24, 32, 16, 20, 12, 28, 1, 2, 262144]
    t = evplp.LIGHTMAP_TEXEL_DTYPE.fields
    assert (t["vpl"][1], t["coverage"][1], t["pm"][1], t["photons"][1]) == (0, 12, 16, 28)


# ---------------------------------------------------------------------------------------------------------------- the twin
def twin(evplp, uv6, W, H, S, x0=0, x1=None, y0=0, y1=None):
    """evplp_lightmap_cover over the texels [x0, x1) x [y0, y1): (inside bool, beta, gamma) as [rows, cols, S, S]"""
    x1 = W if x1 is None else x1; y1 = H if y1 is None else y1
    ins = np.zeros((y1 - y0, x1 - x0, S, S), bool); be = np.zeros(ins.shape, F); ga = np.zeros(ins.shape, F)
    fn = evplp.lib().evplp_lightmap_cover
    uv = np.ascontiguousarray(uv6, F)
    p = uv.ctypes.data_as(C.c_void_p)
    b, g = C.c_float(), C.c_float()
    for y in range(y0, y1):
        for x in range(x0, x1):
            for j in range(S):
                for i in range(S):
                    if fn(p, W, H, S, x, y, i, j, C.byref(b), C.byref(g)):
                        ins[y - y0, x - x0, j, i] = True; be[y - y0, x - x0, j, i] = b.value; ga[y - y0, x - x0, j, i] = g.value
    return ins, be, ga


def restated(uv6, W, H, S, x0=0, x1=None, y0=0, y1=None):
    x1 = W if x1 is None else x1; y1 = H if y1 is None else y1
    px = lr.sample_positions(W, S).reshape(W, S)[x0:x1]; py = lr.sample_positions(H, S).reshape(H, S)[y0:y1]
    return lr.cover_one(uv6, W, H, px[None, :, None, :], py[:, None, :, None])


def agree(evplp, uv6, W, H, S, what, **window):
    a, r = twin(evplp, uv6, W, H, S, **window), restated(uv6, W, H, S, **window)
    assert np.array_equal(a[0], r[0]), (what, S, np.argwhere(a[0] != r[0])[:4])
    assert np.array_equal(a[1].view(np.uint32), r[1].view(np.uint32)) and np.array_equal(a[2].view(np.uint32), r[2].view(np.uint32)), (what, S)
    return a[0]


def SUBPOS(x, i, S):
    """sample i of texel x in sub-texel units; divided by 256 * size it is the texture coordinate, exact for a power-of-two size"""
    return 256 * x + (2 * i + 1) * (128 // S)


@pytest.mark.parametrize("S", (1, 2, 4))
def test_vertices_on_sample_centres_and_edges_through_them_in_eight_directions(evplp, S):
    W = H = 16
    covered = 0
    for d, (dx, dy) in enumerate(DIRS8):
        # an edge from the centre sample of texel (8, 8) along d, four texels long: it passes through sample centres all the way; the third
        # vertex to its left, then to its right (the mirrored chart of the same three points)
        a = np.array([SUBPOS(8, 0, S), SUBPOS(8, 0, S)]); b = a + 4 * 256 * np.array([dx, dy]); c = a + 3 * 256 * np.array([-dy, dx]) + 256 * np.array([dx, dy])
        for tri in ((a, b, c), (a, c, b), (b, a, 2 * a - c), (b, 2 * a - c, a)):
            uv6 = np.array([[p[0] / (256.0 * W), p[1] / (256.0 * H)] for p in tri], F).reshape(6)
            covered += int(agree(evplp, uv6, W, H, S, ("direction", d)).sum())
    assert covered > 100 * S * S
    # two triangles that share the edge: a sample on it belongs to exactly one of them, in every direction
    for d, (dx, dy) in enumerate(DIRS8):
        a = np.array([SUBPOS(8, 0, S), SUBPOS(8, 0, S)]); b = a + 4 * 256 * np.array([dx, dy]); n = 3 * 256 * np.array([-dy, dx])
        left = np.array([[p[0] / (256.0 * W), p[1] / (256.0 * H)] for p in (a, b, a + n)], F).reshape(6)
        right = np.array([[p[0] / (256.0 * W), p[1] / (256.0 * H)] for p in (b, a, a - n)], F).reshape(6)
        l, r = twin(evplp, left, W, H, S)[0], twin(evplp, right, W, H, S)[0]
        assert not (l & r).any(), ("both sides own", d)
        px = lr.sample_positions(W, S).reshape(W, S)[None, :, None, :]; py = lr.sample_positions(H, S).reshape(H, S)[:, None, :, None]
        on = (lr.edge(a[0], a[1], b[0], b[1], px, py) == 0) & ((px - a[0]) * dx + (py - a[1]) * dy > 0) & ((px - b[0]) * dx + (py - b[1]) * dy < 0)
        on = np.broadcast_to(on, l.shape)
        assert on.sum() >= 3 and ((l | r)[on]).all(), ("a sample on the shared edge is nobody's", d, int(on.sum()))


@pytest.mark.parametrize("S", (1, 2, 4))
def test_slivers_outside_uvs_wide_atlases_and_uvs_that_do_not_snap(evplp, S):
    rng = np.random.RandomState(11 + S)
    W, H = 16, 12
    # slivers between two columns of sample centres: thinner than the sample spacing, covering nothing
    step = 256 // S
    x = (SUBPOS(5, 0, S) + 3) / (256.0 * W)
    sliver = np.array([x, 0.1, x + (step - 8) / (256.0 * W), 0.1, x + 4 / (256.0 * W), 0.9], F)
    assert not agree(evplp, sliver, W, H, S, "sliver").any()
    # random triangles, half of them reaching outside [0, 1]^2 (clipped by the atlas: no wrap), both windings as they come
    total = 0
    for k in range(24):
        uv6 = rng.uniform(-0.6, 1.6, 6).astype(F) if k % 2 else rng.uniform(0.0, 1.0, 6).astype(F)
        total += int(agree(evplp, uv6, W, H, S, ("random", k)).sum())
    assert total > 100
    # wholly outside: nothing
    assert not agree(evplp, np.array([1.2, 1.2, 1.9, 1.3, 1.5, 1.8], F), W, H, S, "outside").any()
    assert not agree(evplp, np.array([-0.2, -0.2, -0.9, -0.3, -0.5, -0.8], F), W, H, S, "outside").any()
    # 8192-wide atlases: a small triangle at the far corner, vertices on sample centres and off them, and one that covers the whole window
    W = H = 8192
    for k in range(4):
        base = 8192 - 12
        if k == 0:
            pts = [(SUBPOS(base + 1, 0, S), SUBPOS(base + 1, 0, S)), (SUBPOS(base + 9, S - 1, S), SUBPOS(base + 2, 0, S)), (SUBPOS(base + 4, 0, S), SUBPOS(base + 10, S - 1, S))]
            uv6 = np.array([[p[0] / (256.0 * W), p[1] / (256.0 * H)] for p in pts], F).reshape(6)
        elif k == 3:
            uv6 = np.array([-1.5, 1.2, 1.2, -1.5, 1.2, 1.2], F)
        else:
            uv6 = (1.0 - rng.uniform(0.0, 12.0 / 8192, 6)).astype(F)
        ins = agree(evplp, uv6, W, H, S, ("wide", k), x0=base, x1=8192, y0=base, y1=8192)
        assert ins.any() or k in (1, 2)
        if k == 3:
            assert ins.all()
    # what does not snap is skipped: a NaN, an infinity, a magnitude beyond 2^22 sub-texels; and a triangle of no area
    for bad in (np.nan, np.inf, -np.inf, 3.0e38, 4.0):
        uv6 = np.array([0.1, 0.1, 0.9, 0.2, 0.4, 0.9], F); uv6[3] = bad
        assert not agree(evplp, uv6, 8192, 8192, S, ("bad", bad), x0=800, x1=808, y0=800, y1=808).any()
    assert not agree(evplp, np.array([0.1, 0.1, 0.5, 0.5, 0.9, 0.9], F), 16, 16, S, "no area").any()
    # arguments out of range answer 0
    fn = evplp.lib().evplp_lightmap_cover
    uv = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 1.0], F); b, g = C.c_float(), C.c_float()
    p = uv.ctypes.data_as(C.c_void_p)
    assert fn(p, 16, 16, 1, 2, 2, 0, 0, C.byref(b), C.byref(g)) == 1
    for args in ((0, 16, 1, 0, 0, 0, 0), (16, 8193, 1, 2, 2, 0, 0), (16, 16, 3, 2, 2, 0, 0), (16, 16, 1, 16, 2, 0, 0), (16, 16, 1, 2, -1, 0, 0), (16, 16, 2, 2, 2, 2, 0)):
        assert fn(p, *args, C.byref(b), C.byref(g)) == 0, args
    assert fn(None, 16, 16, 1, 2, 2, 0, 0, C.byref(b), C.byref(g)) == 0


@pytest.mark.parametrize("S", (1, 2, 4))
def test_every_sample_inside_a_mesh_of_triangles_is_covered_exactly_once(evplp, S):
    W = H = 16
    rng = np.random.RandomState(5 + S)
    # a 4 x 4 grid of quads over texels 2 .. 14, every vertex on a sample centre (a random sample of its texel), each quad split along a
    # random diagonal and each triangle wound at random (mirrored charts next to plain ones)
    gx = np.array([[SUBPOS(2 + 3 * i, rng.randint(S), S) for i in range(5)] for _ in range(5)])
    gy = np.array([[SUBPOS(2 + 3 * j, rng.randint(S), S) for _ in range(5)] for j in range(5)])
    # (the outline is kept straight so that "strictly inside the union" is a box test)
    gx[:, 0] = gx[0, 0]; gx[:, 4] = gx[0, 4]; gy[0, :] = gy[0, 0]; gy[4, :] = gy[4, 0]
    tris = []
    for j in range(4):
        for i in range(4):
            q = [(gx[j, i], gy[j, i]), (gx[j, i + 1], gy[j, i + 1]), (gx[j + 1, i + 1], gy[j + 1, i + 1]), (gx[j + 1, i], gy[j + 1, i])]
            pair = ((q[0], q[1], q[2]), (q[0], q[2], q[3])) if rng.rand() < 0.5 else ((q[0], q[1], q[3]), (q[1], q[2], q[3]))
            for t in pair:
                tris.append(t if rng.rand() < 0.5 else (t[0], t[2], t[1]))
    count = np.zeros((H, W, S, S), np.int32)
    for t in tris:
        uv6 = np.array([[p[0] / (256.0 * W), p[1] / (256.0 * H)] for p in t], F).reshape(6)
        count += agree(evplp, uv6, W, H, S, "mesh")
    px = np.broadcast_to(lr.sample_positions(W, S).reshape(W, S)[None, :, None, :], count.shape); py = np.broadcast_to(lr.sample_positions(H, S).reshape(H, S)[:, None, :, None], count.shape)
    inside = (px > gx[0, 0]) & (px < gx[0, 4]) & (py > gy[0, 0]) & (py < gy[4, 0])
    assert inside.sum() > 100 * S * S
    assert (count[inside] == 1).all(), ("a sample inside the union is covered %s times" % sorted(set(count[inside].tolist())))
    assert count.max() == 1 and (count[(px < gx[0, 0]) | (px > gx[0, 4]) | (py < gy[0, 0]) | (py > gy[4, 0])] == 0).all()
    # a fan of eight triangles around a sample centre: the centre belongs to exactly one of them
    c = np.array([SUBPOS(8, S - 1, S), SUBPOS(7, 0, S)])
    ring = [c + 256 * 3 * np.array(d) for d in DIRS8]
    count = np.zeros((H, W, S, S), np.int32)
    for k in range(8):
        t = (c, ring[k], ring[(k + 1) % 8]) if k % 2 else (c, ring[(k + 1) % 8], ring[k])
        uv6 = np.array([[p[0] / (256.0 * W), p[1] / (256.0 * H)] for p in t], F).reshape(6)
        count += agree(evplp, uv6, W, H, S, "fan")
    near = (np.abs(px - c[0]) < 3 * 256) & (np.abs(py - c[1]) < 3 * 256)
    assert (count[near] == 1).all() and count.max() == 1
