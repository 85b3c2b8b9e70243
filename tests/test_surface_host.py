"""No GPU: the surface gather's ABI surface and the host twin of its photon grid (evplp_photon_grid_plan / _cell / _range, the functions
the kernels of kernels_surface.hip call) against the fp32 inside test of evo_photon_frag.

The twin test generates 1.2 million (point, photon, radius, box) cases where the grid can go wrong -- photons at r (1 +- k 2^-23) from the
point along axes and diagonals, points and photons on cell borders +- 1 ulp, radii from 1e-4 to 10 times the box, boxes far from the
origin, points outside the box -- and runs them through a small C program linked against the library (a call per case from Python would
take minutes).  The program evaluates the inside test itself, every operation rounded to fp32 on its own (numpy restates it and must
count the same), and holds the grid to: whenever the test says inside and the photon lies in the box the point is walked; whenever the
test says inside and the point is walked the photon's cell lies in the point's range; a walked point's range is at most 3 cells per axis.
Measured when written: no range wider than 2 cells."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("evplp_gather_surface", "evplp_gather_surface_device", "evplp_photon_grid_plan", "evplp_photon_grid_cell", "evplp_photon_grid_range")


def test_symbols_are_exported_and_declared_and_the_abi_stays_5(evplp):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evplp.h")).read(), flags=re.S)
    lib = C.CDLL(evplp.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in evplp._SIGNATURES, name
    assert lib.evplp_abi_version() == 5 == evplp.ABI_VERSION
    assert evplp.SURFACE_POINT_DTYPE.itemsize == 64 and evplp.SURFACE_LIGHT_DTYPE.itemsize == 32
    assert hasattr(evplp.Context, "gather_surface")


def test_the_surface_structs_have_the_headers_layout(evplp, tmp_path):
    src = tmp_path / "surface_layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "evplp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %u %u %d\\n", sizeof(evplp_surface_point), sizeof(evplp_surface_light), offsetof(evplp_surface_point, valid),
           offsetof(evplp_surface_point, normal), offsetof(evplp_surface_point, rho_d), offsetof(evplp_surface_point, phong_exp),
           offsetof(evplp_surface_light, lit), offsetof(evplp_surface_light, photons), EVPLP_SURFACE_VPL, EVPLP_SURFACE_PHOTONS, EVPLP_SURFACE_CHUNK);
    return 0;
}
''')
    exe = tmp_path / "surface_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [64, 32, 12, 16, 32, 60, 12, 28, evplp.SURFACE_VPL, evplp.SURFACE_PHOTONS, evplp.SURFACE_CHUNK] == [64, 32, 12, 16, 32, 60, 12, 28, 1, 2, 16384]
    p, l = evplp.SURFACE_POINT_DTYPE.fields, evplp.SURFACE_LIGHT_DTYPE.fields
    assert (p["valid"][1], p["normal"][1], p["rho_d"][1], p["rho_s"][1], p["phong_exp"][1]) == (12, 16, 32, 48, 60)
    assert (l["vpl"][1], l["lit"][1], l["pm"][1], l["photons"][1]) == (0, 12, 16, 28)


# ---------------------------------------------------------------------------------------------------------------- the twin
BOXES = [((0.0, 0.0, 0.0), (10.0, 8.0, 5.0)), ((-12.0, -8.0, 0.0), (12.0, 8.0, 90.0)), ((1000.0, -2000.0, 500.0), (1001.0, -1999.0, 500.5)),
         ((-1.0e-3, -1.0e-3, -1.0e-3), (1.0e-3, 2.0e-3, 1.0e-3)), ((-3.0, 4.0, 7.0), (-3.0, 9.0, 7.25))]        # (the last is flat in x)
DIRS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1], [1, -1, 1], [3, 4, 0], [2, 3, 6], [1, 2, 2]], np.float64)
DIRS = np.concatenate([DIRS, -DIRS]); DIRS /= np.linalg.norm(DIRS, axis=1, keepdims=True)


def cases(rng, per_box):
    """float32 [n, 13]: point, photon, radius, box lo, box hi"""
    out = []
    for lo, hi in BOXES:
        lo, hi = np.array(lo), np.array(hi)
        ext = hi - lo; diag = float(np.linalg.norm(ext))
        n = per_box
        r = (diag * 10.0 ** rng.uniform(-4.0, 1.0, n)).astype(F)
        # points: most inside the box, a fifth up to 2 r outside it, a tenth far outside
        x = lo + ext * rng.uniform(0.0, 1.0, (n, 3))
        out_k = rng.rand(n) < 0.2
        x = np.where(out_k[:, None], x + rng.uniform(-2.0, 2.0, (n, 3)) * r[:, None].astype(np.float64) + np.where(rng.rand(n, 3) < 0.5, ext, -ext) * (rng.rand(n, 3) < 0.4), x)
        far = rng.rand(n) < 0.1
        x = np.where(far[:, None], x + rng.uniform(-30.0, 30.0, (n, 3)) * diag, x)
        x = x.astype(F)
        kind = rng.randint(0, 4, n)
        # kind 0: the photon at r (1 +- k 2^-23) from the point along an axis or a diagonal
        k = rng.randint(-8, 9, n).astype(np.float64)
        d = DIRS[rng.randint(0, len(DIRS), n)]
        p_ring = x.astype(np.float64) + d * (r.astype(np.float64) * (1.0 + k * 2.0 ** -23))[:, None]
        # the other kinds: a photon within 1.2 r per axis; on_borders moves it, or the point, onto cell borders
        p_rand = x.astype(np.float64) + rng.uniform(-1.2, 1.2, (n, 3)) * r[:, None].astype(np.float64)
        p = np.where((kind == 0)[:, None], p_ring, p_rand).astype(F)
        row = np.concatenate([x, p, r[:, None], np.broadcast_to(lo.astype(F), (n, 3)), np.broadcast_to(hi.astype(F), (n, 3))], 1).astype(F)
        out.append((row, kind))
    return out


def on_borders(evplp, row, kind, rng):
    """kinds 1 to 3 in place: the photon (1, 3) or the point (2) moved onto lo + m edge +- 1 ulp on every axis, the edge being the plan's;
    kind 3 then puts the point a radius (1 +- k 2^-23) from that photon"""
    n = len(row)
    # one plan per distinct (radius, box) is a call per case: take the plans of 2000 cases and give 60 others each their radius
    pick = rng.randint(0, n, 2000)
    for i in pick:
        plan = evplp.photon_grid_plan(float(row[i, 6]), row[i, 7:10], row[i, 10:13], 1000)
        assert plan is not None, row[i]
        edge = plan[0]
        take = np.nonzero(kind != 0)[0]
        take = take[rng.randint(0, len(take), 60)]
        row[take, 6] = row[i, 6]
        lo = row[i, 7:10].astype(np.float64)
        for j in take:
            col = slice(3, 6) if kind[j] in (1, 3) else slice(0, 3)
            m = np.round((row[j, col].astype(np.float64) - lo) / edge)
            b = (lo + m * float(edge)).astype(F)
            step = rng.randint(-1, 2, 3)
            b = np.where(step > 0, np.nextafter(b, F(np.inf)), np.where(step < 0, np.nextafter(b, F(-np.inf)), b))
            row[j, col] = b
            if kind[j] == 3:        # ... and the point a radius (1 +- k 2^-23) from that photon along an axis
                ax = rng.randint(0, 3); sgn = 1.0 if rng.rand() < 0.5 else -1.0
                x = row[j, 3:6].astype(np.float64)
                x[ax] += sgn * float(row[j, 6]) * (1.0 + rng.randint(-8, 9) * 2.0 ** -23)
                row[j, 0:3] = x.astype(F)


DRIVER = r'''
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include "evplp.h"
int main(int argc, char **argv) {
    FILE *f = fopen(argv[1], "rb"); long n = atol(argv[2]);
    float *c = (float *)malloc(sizeof(float) * 13 * (size_t)n);
    if (!f || fread(c, sizeof(float) * 13, (size_t)n, f) != (size_t)n) return 2;
    long inside = 0, refused = 0, miss_walk = 0, miss_cell = 0, walked = 0, wide3 = 0, wide2 = 0; int widest = 0;
    for (long i = 0; i < n; i++) {
        const float *x = c + 13 * i, *p = x + 3, r = x[6], *lo = x + 7, *hi = x + 10;
        float edge; uint32_t bits;
        if (evplp_photon_grid_plan(r, lo, hi, 1000u, &edge, &bits) != EVPLP_OK) { refused++; continue; }
        /* evo_photon_frag's test, every operation rounded to fp32 on its own (built without contraction) */
        volatile float dx = p[0] - x[0], dy = p[1] - x[1], dz = p[2] - x[2];
        volatile float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        volatile float xy = xx + yy; volatile float d2 = xy + zz; volatile float r2 = r * r;
        const int in = !(d2 > r2);
        int32_t cell[3], c0[3], c1[3];
        evplp_photon_grid_cell(p, lo, edge, bits, cell);
        const int walk = evplp_photon_grid_range(x, r, lo, hi, edge, c0, c1);
        int in_box = 1, in_range = 1;
        for (int k = 0; k < 3; k++) { if (p[k] < lo[k] || p[k] > hi[k]) in_box = 0; if (cell[k] < c0[k] || cell[k] > c1[k]) in_range = 0; }
        inside += in; walked += walk;
        if (in && in_box && !walk) miss_walk++;
        if (in && walk && !in_range) miss_cell++;
        if (walk) for (int k = 0; k < 3; k++) { const int w = c1[k] - c0[k] + 1; if (w > widest) widest = w; if (w > 3) wide3++; if (w > 2) wide2++; }
    }
    printf("%ld %ld %ld %ld %ld %ld %ld %d\n", inside, refused, miss_walk, miss_cell, walked, wide3, wide2, widest);
    return 0;
}
'''


def test_the_range_holds_every_photon_the_fp32_test_calls_inside(evplp, tmp_path):
    rng = np.random.RandomState(20266)
    parts = cases(rng, 240000)
    for row, kind in parts:
        on_borders(evplp, row, kind, rng)
    rows = np.ascontiguousarray(np.concatenate([r for r, _ in parts]), F)
    n = len(rows)
    assert n >= 1000000
    data = tmp_path / "cases.f32"; rows.tofile(str(data))
    src = tmp_path / "grid_cases.c"; src.write_text(DRIVER)
    exe = tmp_path / "grid_cases"
    libdir = os.path.dirname(evplp.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-O1", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                    "-L", libdir, "-l:" + os.path.basename(evplp.LIB_PATH), "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe), str(data), str(n)], capture_output=True, text=True, check=True).stdout.split()
    inside, refused, miss_walk, miss_cell, walked, wide3, wide2, widest = [int(v) for v in out]
    # numpy's float32 arithmetic rounds every operation on its own too: the same count
    x, p, r = rows[:, 0:3], rows[:, 3:6], rows[:, 6]
    dv = p - x
    d2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
    assert d2.dtype == F and int((~(d2 > r * r)).sum()) == inside
    print(f"\nphoton grid: {n} cases, {inside} inside, {walked} points walked, ranges wider than 2 cells: {wide2}, widest {widest}")
    assert refused == 0, "the plan refuses nothing of these"
    assert inside > 0.2 * n and n - inside > 0.2 * n and walked > 0.5 * n and n - walked > 0.05 * n
    assert miss_walk == 0 and miss_cell == 0, (miss_walk, miss_cell)
    assert wide3 == 0 and widest <= 3


def test_the_cases_sit_where_the_test_is_decided_by_an_ulp(evplp):
    """what the generator is for: among the ring cases both answers of the inside test occur within 8 ulp of r"""
    rng = np.random.RandomState(5)
    row, kind = cases(rng, 20000)[0]
    ring = kind == 0
    dv = row[ring, 3:6] - row[ring, 0:3]
    d2 = (dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2]
    r = row[ring, 6]
    rel = np.sqrt(d2.astype(np.float64)) / r - 1.0
    near = np.abs(rel) < 1e-5
    inside = ~(d2 > r * r)
    assert near.mean() > 0.5 and inside[near].sum() > 500 and (~inside[near]).sum() > 500


def test_plan_is_monotone_and_refuses_only_what_it_should(evplp):
    lo, hi = (0.0, 0.0, 0.0), (10.0, 8.0, 5.0)
    last = 0
    for usable in (0, 1, 15, 16, 17, 1000, 1 << 16, (1 << 16) + 1, 2000000, 1 << 24, (1 << 24) + 1, 0xffffffff):
        edge, bits = evplp.photon_grid_plan(0.1, lo, hi, usable)
        assert 4 <= bits <= 24 and bits >= last and ((1 << bits) >= usable or bits == 24), (usable, bits)
        last = bits
    last = 0.0
    diag = float(np.linalg.norm(hi))
    for r in diag * 10.0 ** np.linspace(-4.0, 1.0, 41):
        plan = evplp.photon_grid_plan(float(F(r)), lo, hi, 1000)
        assert plan is not None, r
        assert plan[0] >= last and plan[0] >= 2.0 * float(F(r)), (r, plan)
        last = plan[0]
    assert evplp.photon_grid_plan(1e-30, lo, hi, 10) is not None and evplp.photon_grid_plan(1e30, lo, hi, 10) is not None
    assert evplp.photon_grid_plan(0.1, lo, lo, 10) is not None, "a box without extent"
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert evplp.photon_grid_plan(r, lo, hi, 10) is None, r
    assert evplp.photon_grid_plan(0.1, hi, lo, 10) is None and evplp.photon_grid_plan(0.1, (float("nan"), 0, 0), hi, 10) is None
    assert evplp.photon_grid_plan(0.1, lo, (float("inf"), 8.0, 5.0), 10) is None
    # the Python wrappers give what the C functions give
    edge, bits = evplp.photon_grid_plan(0.25, lo, hi, 5000)
    cell, bucket = evplp.photon_grid_cell((5.0, 4.0, 2.5), lo, edge, bits)
    walked, c0, c1 = evplp.photon_grid_range((5.0, 4.0, 2.5), 0.25, lo, hi, edge)
    assert walked and (c0 <= cell).all() and (cell <= c1).all() and 0 <= bucket < (1 << bits)
    assert not evplp.photon_grid_range((50.0, 4.0, 2.5), 0.25, lo, hi, edge)[0]
