"""No GPU: the probe gather's ABI surface and its host twin (evplp_probe_pair, evplp_sh_basis, evplp_sh_irradiance) against the float64
restatement of tests/probe_restate.py.

evplp_probe_pair is compared on every record of shading_domain.make_vpls() x probe positions that visit: in front of the VPL (a grid on
and above the floor), behind its plane (exactly 0), inside min_distance (the clamp), at the VPL itself (exactly 0), and on and off each
Phong lobe -- under
    |x - f64| <= (K 2^-24 kappa) |f64| + 1e-20        on decided pairs          (shading_domain.bar, hw_pow=False: the twin takes libm's powf)
K_ORACLE_PROBE is the smallest integer that held when measured; the GPU test (test_gpu_probe.py) grants the kernel twice that."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import probe_restate as pr
import shading_domain as sd
from probe_domain import K_ORACLE_PROBE, MIN_DISTANCE, positions_for      # noqa: F401  (test_gpu_probe.py takes K_ORACLE_PROBE from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

def test_symbols_are_exported_and_declared_and_the_abi_stays_5(evplp):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evplp.h")).read(), flags=re.S)
    lib = C.CDLL(evplp.LIB_PATH)
    for name in ("evplp_gather_probes", "evplp_gather_probes_device", "evplp_probe_pair", "evplp_sh_basis", "evplp_sh_irradiance"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name) and name in evplp._SIGNATURES, name
    assert lib.evplp_abi_version() == 5 == evplp.ABI_VERSION
    assert evplp.PROBE_SH_DTYPE.itemsize == 112 and C.sizeof(evplp.ProbeParams) == 16


def test_the_probe_structs_have_the_headers_layout(evplp, tmp_path):
    src = tmp_path / "probe_layout.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "evplp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(evplp_probe_sh), offsetof(evplp_probe_sh, lit), sizeof(evplp_probe_params), offsetof(evplp_probe_params, min_distance),
           offsetof(evplp_probe_params, flags), EVPLP_PROBE_CHUNK, EVPLP_PROBE_SLICE_SLOTS);
    return 0;
}
''')
    exe = tmp_path / "probe_layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [112, 108, 16, 8, 12, evplp.PROBE_CHUNK, evplp.PROBE_SLICE_SLOTS] == [112, 108, 16, 8, 12, 16384, 256]
    assert evplp.PROBE_SH_DTYPE.fields["lit"][1] == 108 and evplp.ProbeParams.min_distance.offset == 8 and evplp.ProbeParams.flags.offset == 12


def sphere_quadrature(nz=64, nphi=128):
    """Gauss-Legendre in z times the trapezoid in phi: exact for polynomials of degree < 2 nz in z and < nphi in the azimuth"""
    z, wz = np.polynomial.legendre.leggauss(nz)
    phi = 2.0 * np.pi * (np.arange(nphi) + 0.5) / nphi
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s[:, None] * np.cos(phi)[None, :], s[:, None] * np.sin(phi)[None, :], np.broadcast_to(z[:, None], (nz, nphi))], -1).reshape(-1, 3)
    return d, np.repeat(wz, nphi) * (2.0 * np.pi / nphi)


def test_the_restated_basis_is_orthonormal_over_the_sphere():
    d, w = sphere_quadrature()
    assert abs(w.sum() - 4.0 * np.pi) < 1e-12
    Y = pr.basis_exact(d)
    gram = (Y * w[:, None]).T @ Y
    assert np.abs(gram - np.eye(9)).max() < 1e-12, gram
    # the header's eight digits are those constants rounded, and basis_f64 is the same polynomials with them
    assert np.abs(pr.basis_f64(d) - Y).max() < 1e-7
    # the irradiance weights: the clamped cosine around +z projected on the zonal functions Y0, Y2, Y6, times sqrt(4 pi / (2 l + 1)).
    # Over the upper hemisphere alone the integrand is a polynomial in z: 2 pi int_0^1 z Y_l0(z) dz, exact under Gauss-Legendre on [0, 1]
    z, wz = np.polynomial.legendre.leggauss(8)
    z, wz = 0.5 * (z + 1.0), 0.5 * wz
    zonal = pr.basis_exact(np.stack([np.sqrt(1.0 - z * z), np.zeros_like(z), z], -1))
    for l, i in ((0, 0), (1, 2), (2, 6)):
        a_l = np.sqrt(4.0 * np.pi / (2 * l + 1)) * 2.0 * np.pi * (wz * z * zonal[:, i]).sum()
        assert abs(a_l - pr.BAND[i]) < 1e-12, (l, a_l, pr.BAND[i])


def test_sh_basis_and_irradiance_match_the_restatement(evplp):
    rng = np.random.RandomState(4)
    dirs = rng.normal(size=(500, 3)); dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    dirs = np.concatenate([dirs, np.eye(3), -np.eye(3), [[0.6, 0.8, 0.0], [0.0, 0.0, 0.0], [2.0, -3.0, 0.5]]]).astype(F)    # (not normalised: taken as given)
    worst = 0.0
    for d in dirs:
        got = evplp.sh_basis(d).astype(np.float64)
        want, mag = pr.basis_f64(d), pr.basis_abs_f64(d)
        err = np.abs(got - want)
        assert (err <= 4 * 2.0 ** -24 * mag).all(), (d, got, want)          # at most four roundings (Y6: z z, 3 x, - 1, the constant), each 2^-24 of a term
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()) / 2.0 ** -24)
    print(f"\nsh_basis: worst error {worst:.2f} x 2^-24 of the terms' magnitudes")
    worst = 0.0
    for k, n in enumerate(dirs[:200]):
        sh = np.zeros(1, evplp.PROBE_SH_DTYPE)
        sh["c"][0] = (rng.normal(size=(9, 3)) * (10.0 ** rng.uniform(-3, 1))).astype(F)
        sh["lit"][0] = 7.0
        got = evplp.sh_irradiance(sh[0], n).astype(np.float64)
        want, mag = pr.irradiance_f64(sh["c"][0], n), pr.irradiance_abs_f64(sh["c"][0], n)
        err = np.abs(got - want)
        assert (err <= 14 * 2.0 ** -24 * mag).all(), (n, got, want)      # per term: four roundings of Y_i, the band weight, the coefficient; eight sums
        worst = max(worst, float((err / mag).max()) / 2.0 ** -24)
    print(f"sh_irradiance: worst error {worst:.2f} x 2^-24 of the sum of the terms' magnitudes")
    # a constant environment L: c0 = L / Y0 ... irradiance pi L on any normal
    sh = np.zeros(1, evplp.PROBE_SH_DTYPE); sh["c"][0, 0] = (2.0 / 0.28209479, 1.0 / 0.28209479, 0.0)
    assert np.allclose(evplp.sh_irradiance(sh[0], [0.0, 0.6, 0.8]), [2.0 * np.pi, np.pi, 0.0], rtol=1e-6)


def test_probe_pair_obeys_the_bar_on_every_record_and_kind_of_position(evplp):
    recs, names = sd.make_vpls()
    recs = recs.astype(evplp.RECORD_DTYPE)
    worst, und, facing_pairs, seen = 0.0, [], 0, {}
    for k, name in enumerate(names):
        X, kinds = positions_for(recs[k])
        term, kappa, lam, decided, facing = pr.pair_f64(recs[k], X, MIN_DISTANCE)
        got = np.stack([evplp.probe_pair(recs[k], x, MIN_DISTANCE) for x in X]).astype(np.float64)
        assert np.isfinite(got).all(), name
        f32_facing, _ = pr.facing_f32(recs[k], X)
        assert (f32_facing == facing)[decided].all(), name
        assert (got[~f32_facing] == 0.0).all(), (name, "no term without the cosine test")
        assert (got[kinds == "behind"] == 0.0).all() and (got[kinds == "at_vpl"] == 0.0).all(), name
        ok = np.abs(got - term) <= sd.bar(term, kappa, lam, K_ORACLE_PROBE, False)
        bad = np.argwhere(~ok.all(axis=(1, 2)) & decided)
        ratio = sd.worst_ratio(got.reshape(len(X), 27), term.reshape(len(X), 27), np.broadcast_to(kappa, term.shape).reshape(len(X), 27), lam[:, 0], decided)
        worst = max(worst, ratio)
        assert bad.size == 0, (name, ratio, kinds[bad[0, 0]], X[bad[0, 0]], got[bad[0, 0]], term[bad[0, 0]])
        if name == "zero_flux":                   # (the other dark records of the floor tests do light a probe in front of them)
            assert (got == 0.0).all(), name
        und.append(int((~decided & facing).sum())); facing_pairs += int(facing.sum())
        # what the positions are meant to visit
        inside = kinds == "inside_min_distance"
        d2 = ((recs[k]["pos"].astype(np.float64) - X[inside].astype(np.float64)) ** 2).sum(-1)
        assert (d2 < MIN_DISTANCE ** 2).all(), name
        lit = np.abs(got).sum(axis=(1, 2)) > 0
        for kind in np.unique(kinds):
            seen[kind] = seen.get(kind, 0) + int(lit[kinds == kind].sum())
        if np.any(recs[k]["rho_s"] != 0) and facing[kinds == "on_lobe"].any():        # a record whose lobe some probe on its axis takes
            seen["lobe_term"] = seen.get("lobe_term", 0) + int((lam[kinds == "on_lobe"] > 0).any() or recs[k]["phong_exp"] == 0)
    caps = sd.check_caps(und, facing_pairs)
    print(f"\nprobe_pair: worst error / (2^-24 kappa |f64|) = {worst:.2f} over {len(names)} records, {facing_pairs} facing pairs; undecided: worst record {caps[0]}, all {caps[1]}; lit by kind {seen}")
    assert seen["grid"] > 5000 and seen["inside_min_distance"] > 20 and seen["on_lobe"] > 20 and seen["lobe_flank"] > 20 and seen["lobe_term"] >= 8
    assert seen["behind"] == 0 and seen["at_vpl"] == 0
    assert worst <= K_ORACLE_PROBE
