"""No GPU needed: the per-point state of the progressive surface gather (include/evplp.h "progressive surface gather").  The symbols are
exported, declared and bound at ABI 5; the state's layout against the header by a compiled C program; and the two host-only entry points
-- evplp_surface_state_update and evplp_surface_state_resolve, the functions of surface_state.h that the kernels call -- against a numpy
float32 restatement, BIT FOR BIT, over a table of cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("evplp_gather_surface_progressive", "evplp_gather_surface_progressive_device", "evplp_surface_resolve", "evplp_surface_resolve_device",
       "evplp_bake_lightmap_progressive_device", "evplp_bake_lightmap_resolve", "evplp_bake_lightmap_resolve_device", "evplp_surface_state_update",
       "evplp_surface_state_resolve")
INV_PI = F(0.318309886183790671537767526745028724068919291480912897495)


def test_the_symbols_are_exported_declared_and_bound_at_abi_5(evplp):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evplp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(evplp_[a-z_0-9]+)\s*\(", hdr))
    lib = C.CDLL(evplp.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in evplp._SIGNATURES, name
    assert lib.evplp_abi_version() == 5 == evplp.ABI_VERSION
    for name in ("gather_surface_progressive", "surface_resolve", "bake_lightmap_progressive_device", "bake_lightmap_resolve", "bake_lightmap_resolve_device"):
        assert callable(getattr(evplp.Context, name)), name
    assert evplp.SURFACE_STATE_DTYPE.itemsize == 48 and evplp.STATE_INVALID == 1


def test_the_state_is_48_bytes_with_the_headers_offsets(evplp, tmp_path):
    src = tmp_path / "state.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "evplp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u\\n", sizeof(evplp_surface_state), offsetof(evplp_surface_state, tau), offsetof(evplp_surface_state, radius2),
           offsetof(evplp_surface_state, vpl), offsetof(evplp_surface_state, n), offsetof(evplp_surface_state, lit_sum), offsetof(evplp_surface_state, vpl_calls),
           offsetof(evplp_surface_state, pm_calls), offsetof(evplp_surface_state, flags), (unsigned)EVPLP_STATE_INVALID);
    return 0;
}
''')
    exe = tmp_path / "state"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    d = evplp.SURFACE_STATE_DTYPE
    assert got == [48] + [d.fields[k][1] for k in ("tau", "radius2", "vpl", "n", "lit_sum", "vpl_calls", "pm_calls", "flags")] + [evplp.STATE_INVALID]
    assert got[1:9] == [0, 12, 16, 28, 32, 36, 40, 44]


# ---------------------------------------------------------------------------------------------------------------- the restatement
def restate_update(state, m, phi, alpha, r0sq):
    """include/evplp.h's rule in numpy float32 scalars: every operation rounded to fp32 on its own, IEEE division"""
    s = state.copy()
    alpha, r0sq, phi = F(alpha), F(r0sq), np.asarray(phi, F)
    r2 = s["radius2"][0]
    if s["pm_calls"][0] > 0 and not (np.isfinite(r2) and r2 > 0 and r2 <= r0sq):
        s["flags"] |= 1
        return s
    if s["pm_calls"][0] == 0:
        s["radius2"][0] = r0sq
    if m > 0:
        mf = F(m)
        n = s["n"][0]
        nn = F(n + F(alpha * mf))
        ratio = F(nn / F(n + mf))
        s["radius2"][0] = F(s["radius2"][0] * ratio)
        for k in range(3):
            s["tau"][0, k] = F(F(s["tau"][0, k] + phi[k]) * ratio)
        s["n"][0] = nn
    s["pm_calls"] += 1
    return s


def restate_resolve(evplp, state):
    out = np.zeros(1, evplp.SURFACE_LIGHT_DTYPE)
    s = state
    if s["flags"][0] & 1:
        out["lit"] = -1; out["photons"] = -1
        return out
    with np.errstate(all="ignore"):
        if s["vpl_calls"][0] > 0:
            d = F(s["vpl_calls"][0])
            out["vpl"][0] = (s["vpl"][0] / d).astype(F); out["lit"][0] = F(s["lit_sum"][0] / d)
        if s["pm_calls"][0] > 0:
            d = F(s["radius2"][0] * F(s["pm_calls"][0]))
            for k in range(3):
                out["pm"][0, k] = F(F(s["tau"][0, k] * INV_PI) / d)
            out["photons"][0] = s["n"][0]
    return out


def state_of(evplp, **kw):
    s = np.zeros(1, evplp.SURFACE_STATE_DTYPE)
    for k, v in kw.items():
        s[k][0] = v
    return s


def tiny(x):
    return float(F(x))


# (name, the state's fields, M, phi, alpha, r0sq)
CASES = [
    ("fresh", {}, 5, (0.25, 0.5, 0.125), 2.0 / 3.0, 0.09),
    ("fresh, M = 0", {}, 0, (0.0, 0.0, 0.0), 2.0 / 3.0, 0.09),
    ("fresh, M = 1", {}, 1, (0.3, 0.2, 0.1), 0.7, 0.0123),
    ("M = 0 keeps tau, radius2 and n", dict(tau=(1.5, 2.5, 3.5), radius2=0.01, n=12.25, pm_calls=3, vpl=(1, 2, 3), lit_sum=9, vpl_calls=2), 0, (7.0, 7.0, 7.0), 0.5, 0.02),
    ("M = 1", dict(tau=(1.5, 2.5, 3.5), radius2=0.01, n=12.25, pm_calls=3), 1, (0.1, 0.2, 0.3), 2.0 / 3.0, 0.02),
    ("alpha = 1: ratio is exactly 1", dict(tau=(1.5, 2.5, 3.5), radius2=0.0131, n=1234.0, pm_calls=7), 17, (0.1, 0.2, 0.3), 1.0, 0.0131),
    ("alpha = 1, fresh", {}, 3, (0.1, 0.2, 0.3), 1.0, 0.0131),
    ("n absorbs alpha M", dict(tau=(1e3, 2e3, 3e3), radius2=1e-4, n=2.0 ** 25, pm_calls=900), 3, (0.1, 0.2, 0.3), 0.3, 0.01),
    ("n absorbs M too", dict(tau=(1e3, 2e3, 3e3), radius2=1e-4, n=2.0 ** 26, pm_calls=900), 1, (0.1, 0.2, 0.3), 0.9, 0.01),
    ("radius2 denormal", dict(tau=(1e-3, 2e-3, 3e-3), radius2=tiny(3e-42), n=40.0, pm_calls=5), 2, (1e-5, 2e-5, 3e-5), 2.0 / 3.0, 0.01),
    ("radius2 the smallest denormal", dict(tau=(1e-3, 2e-3, 3e-3), radius2=tiny(1.4e-45), n=1.0, pm_calls=1), 9, (1e-5, 2e-5, 3e-5), 0.1, 0.01),
    ("radius2 equals r0sq", dict(radius2=tiny(0.09), n=3.0, pm_calls=1), 4, (0.1, 0.2, 0.3), 0.5, tiny(0.09)),
    ("many photons", dict(tau=(0.5, 0.5, 0.5), radius2=0.003, n=77.7, pm_calls=2), 100000, (31.0, 32.0, 33.0), 2.0 / 3.0, 0.01),
    # out of range with pm_calls > 0: flagged, every other byte kept
    ("invalid: radius2 one ulp above r0sq", dict(tau=(1, 2, 3), radius2=float(np.nextafter(F(0.09), F(1))), n=3.0, pm_calls=1), 4, (0.1, 0.2, 0.3), 0.5, tiny(0.09)),
    ("invalid: radius2 = 0", dict(tau=(1, 2, 3), radius2=0.0, n=3.0, pm_calls=1), 4, (0.1, 0.2, 0.3), 0.5, 0.09),
    ("invalid: radius2 < 0", dict(tau=(1, 2, 3), radius2=-0.01, n=3.0, pm_calls=1), 4, (0.1, 0.2, 0.3), 0.5, 0.09),
    ("invalid: radius2 NaN", dict(tau=(1, 2, 3), radius2=float("nan"), n=3.0, pm_calls=2), 4, (0.1, 0.2, 0.3), 0.5, 0.09),
    ("invalid: radius2 inf", dict(tau=(1, 2, 3), radius2=float("inf"), n=3.0, pm_calls=2), 4, (0.1, 0.2, 0.3), 0.5, 0.09),
    # pm_calls == 0: whatever radius2 holds is replaced
    ("garbage radius2 before the first photon half", dict(radius2=float("nan"), vpl=(1, 2, 3), lit_sum=5, vpl_calls=1), 2, (0.1, 0.2, 0.3), 0.5, 0.09),
    ("already flagged: the rule still applies, the resolve answers -1", dict(tau=(1, 2, 3), radius2=0.01, n=3.0, pm_calls=1, flags=1), 4, (0.1, 0.2, 0.3), 0.5, 0.09),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_update_and_resolve_match_the_float32_restatement_bit_for_bit(evplp, case):
    name, fields, m, phi, alpha, r0sq = case
    before = state_of(evplp, **fields)
    got = evplp.surface_state_update(before, m, phi, alpha, r0sq)
    want = restate_update(before, m, phi, alpha, r0sq)
    assert got.tobytes() == want.tobytes(), (name, got, want)
    if name.startswith("invalid"):
        assert got["flags"][0] == 1
        keep = before.copy(); keep["flags"] = 1
        assert got.tobytes() == keep.tobytes(), name + ": a flagged state keeps every other byte"
    elif m == 0:
        assert got["tau"].tobytes() == before["tau"].tobytes() and got["n"].tobytes() == before["n"].tobytes() and got["pm_calls"][0] == before["pm_calls"][0] + 1
        if before["pm_calls"][0] > 0:
            assert got["radius2"].tobytes() == before["radius2"].tobytes()
    else:
        start = F(r0sq) if before["pm_calls"][0] == 0 else before["radius2"][0]
        assert got["radius2"][0] <= start, name + ": a radius never grows"
        if alpha == 1.0:
            assert got["radius2"].tobytes() == np.asarray([start], F).tobytes() and got["n"][0] == F(before["n"][0] + F(m))
    assert got["vpl"].tobytes() == before["vpl"].tobytes() and got["lit_sum"][0] == before["lit_sum"][0] and got["vpl_calls"][0] == before["vpl_calls"][0]
    for s in (before, got):
        assert evplp.surface_state_resolve(s).tobytes() == restate_resolve(evplp, s).tobytes(), (name, s)


def test_a_fresh_state_resolves_to_32_zero_bytes_and_a_flagged_one_to_minus_one(evplp):
    assert evplp.surface_state_resolve(np.zeros(1, evplp.SURFACE_STATE_DTYPE)).tobytes() == bytes(32)
    s = state_of(evplp, tau=(1, 2, 3), radius2=0.5, vpl=(4, 5, 6), n=7, lit_sum=8, vpl_calls=2, pm_calls=3, flags=1)
    assert evplp.surface_state_resolve(s).view(F).tolist() == [0, 0, 0, -1, 0, 0, 0, -1]
    s["flags"] = 0
    r = evplp.surface_state_resolve(s)
    assert r["vpl"][0].tolist() == [2.0, 2.5, 3.0] and r["lit"][0] == 4.0 and r["photons"][0] == 7.0
    assert r["pm"][0].tobytes() == np.asarray([F(F(t * INV_PI) / F(1.5)) for t in (F(1), F(2), F(3))], F).tobytes()
    s["vpl_calls"] = 0
    r = evplp.surface_state_resolve(s)
    assert (r["vpl"] == 0).all() and r["lit"][0] == 0 and r["photons"][0] == 7.0


def test_a_chain_of_iterations_shrinks_the_radius_and_matches_the_restatement(evplp):
    rng = np.random.RandomState(11)
    for alpha in (2.0 / 3.0, 0.5, 1.0, 0.01):
        a = b = np.zeros(1, evplp.SURFACE_STATE_DTYPE)
        last = F(0.04)
        for it in range(40):
            m = int(rng.randint(0, 50)) if it % 5 else 0
            phi = rng.rand(3).astype(F) * F(m)
            a = evplp.surface_state_update(a, m, phi, alpha, 0.04)
            b = restate_update(b, m, phi, alpha, 0.04)
            assert a.tobytes() == b.tobytes(), (alpha, it)
            assert a["radius2"][0] <= last and (m == 0 or alpha == 1.0 or a["radius2"][0] < last), (alpha, it, m)
            last = a["radius2"][0]
        assert a["pm_calls"][0] == 40 and a["flags"][0] == 0
