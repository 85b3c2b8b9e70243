"""No GPU needed: the select and the seed behind the k-nearest-photon start radius (include/evplp.h "k-nearest-photon start radii").  The
symbols are exported, declared and bound at ABI 5; evplp_knn_params' layout by a compiled C program; evplp_knn_radius2 -- knn_select.h's
radix select, the functions surface_knn_select_kernel calls -- against np.sort on float32 arrays, BIT FOR BIT, on sets built to break a
radix select (ties around the k-th, neighbours one ulp apart, values that differ in one nibble only, zeros and denormals, values that are
no candidates, both clamps); evplp_surface_state_seed -- surface_state.h's ss_seed -- against a numpy float32 restatement, bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("evplp_gather_surface_knn", "evplp_gather_surface_knn_device", "evplp_bake_lightmap_knn_device", "evplp_knn_radius2", "evplp_surface_state_seed")
R0SQ = F(0.25)
RMINSQ = F(2.0 ** -60)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def from_bits(u):
    return np.asarray(u, np.uint32).view(F)


def test_the_symbols_are_exported_declared_and_bound_at_abi_5(evplp):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evplp.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(evplp_[a-z_0-9]+)\s*\(", hdr))
    lib = C.CDLL(evplp.LIB_PATH)
    for name in NEW:
        assert name in declared and hasattr(lib, name) and name in evplp._SIGNATURES, name
    assert lib.evplp_abi_version() == 5 == evplp.ABI_VERSION
    for name in ("gather_surface_knn", "bake_lightmap_knn"):
        assert callable(getattr(evplp.Context, name)), name
    assert callable(evplp.knn_radius2) and callable(evplp.surface_state_seed)
    assert C.sizeof(evplp.KnnParams) == 16


def test_the_params_are_16_bytes_with_the_headers_offsets(evplp, tmp_path):
    src = tmp_path / "knn.c"
    src.write_text('''#include <stdio.h>
#include <stddef.h>
#include "evplp.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu\\n", sizeof(evplp_knn_params), offsetof(evplp_knn_params, k), offsetof(evplp_knn_params, r_min),
           offsetof(evplp_knn_params, alpha), offsetof(evplp_knn_params, flags));
    return 0;
}
''')
    exe = tmp_path / "knn"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [16, 0, 4, 8, 12]
    assert got[1:] == [getattr(evplp.KnnParams, f).offset for f in ("k", "r_min", "alpha", "flags")]


# ---------------------------------------------------------------------------------------------------------------- the select
def by_sort(d2, k, rminsq, r0sq):
    """include/evplp.h's definition with np.sort: (rk2, M)"""
    d2 = np.asarray(d2, F).reshape(-1)
    cand = np.sort(d2[~(d2 > r0sq)])
    kth = cand[k - 1] if len(cand) >= k else F(r0sq)
    rk2 = min(max(kth, F(rminsq)), F(r0sq))
    return F(rk2), int((~(cand > rk2)).sum())


def check(evplp, d2, k, rminsq=RMINSQ, r0sq=R0SQ, what=""):
    d2 = np.asarray(d2, F).reshape(-1)
    got, m = evplp.knn_radius2(d2, k, rminsq, r0sq)
    want, wm = by_sort(d2, k, rminsq, r0sq)
    assert bits(got)[()] == bits(want)[()] and m == wm, (what, k, len(d2), got, want, m, wm)
    return got, m


def ladder(start, n):
    """n consecutive floats from start upwards"""
    return from_bits(bits(F(start))[()] + np.arange(n, dtype=np.uint32))


def test_k_at_the_ends_and_the_empty_set(evplp):
    rng = np.random.RandomState(1)
    d2 = (rng.rand(37).astype(F) * R0SQ).astype(F)
    assert (d2 > RMINSQ).all()
    for k in (1, 2, 36, 37):
        got, m = check(evplp, d2, k, what="ends")
        assert bits(got)[()] == bits(np.sort(d2)[k - 1])[()] and m == k
    assert check(evplp, d2, 38, what="k = count + 1") == (R0SQ, 37)
    assert check(evplp, d2, 2 ** 24, what="k far above") == (R0SQ, 37)
    assert check(evplp, np.zeros(0, F), 1, what="count = 0") == (R0SQ, 0)
    assert check(evplp, d2[:1], 1, what="one") == (d2[0], 1)


def test_ties(evplp):
    v = F(0.0123)
    same = np.full(9, v, F)
    for k in (1, 5, 9):
        assert check(evplp, same, k, what="all equal") == (v, 9)
    assert check(evplp, same, 10, what="all equal, k above") == (R0SQ, 9)
    # k - 1 ties below the k-th
    k = 6
    d2 = np.concatenate([np.full(k - 1, F(0.001), F), [F(0.002)], [F(0.003), F(0.2)]]).astype(F)
    assert check(evplp, d2, k, what="k - 1 ties below") == (F(0.002), k)
    assert check(evplp, d2, k - 1, what="the last of the ties") == (F(0.001), k - 1)
    # ties straddling the k-th: M > k
    d2 = np.asarray([0.001, 0.002, 0.002, 0.002, 0.002, 0.003], F)
    for k in (2, 3, 4, 5):
        assert check(evplp, d2, k, what="straddling") == (F(0.002), 5)
    assert check(evplp, d2[::-1].copy(), 3, what="straddling, reversed") == (F(0.002), 5)


def test_neighbours_one_ulp_apart(evplp):
    for start in (0.0123, 2.0 ** -7, float(np.nextafter(F(2.0 ** -7), F(0))), 2.0 ** -126, 1e-42):
        d2 = ladder(start, 40)
        rng = np.random.RandomState(2)
        rng.shuffle(d2)
        for k in (1, 2, 16, 17, 39, 40):
            got, m = check(evplp, d2, k, rminsq=F(2.0 ** -140), what=f"ulp ladder from {start}")
            assert m == k and bits(got)[()] == bits(F(start))[()] + k - 1


def test_values_that_differ_in_one_nibble_only(evplp):
    base = bits(F(0.0123))[()] & ~np.uint32(0xF)
    low = from_bits(base + np.arange(16, dtype=np.uint32))           # the lowest nibble: the last pass decides
    for k in range(1, 17):
        got, m = check(evplp, low[::-1].copy(), k, what="lowest nibble")
        assert bits(got)[()] == base + k - 1 and m == k
    top = from_bits((np.arange(0, 4, dtype=np.uint32) << 28) | np.uint32(0x00ABCDEF))       # the top nibble: pass 0 decides (0x3... is 2^-31 or so)
    top = top[~(top > R0SQ)]
    assert len(top) == 4
    for k in range(1, 5):
        got, m = check(evplp, top[::-1].copy(), k, rminsq=F(2.0 ** -140), what="top nibble")
        assert bits(got)[()] == bits(top)[k - 1] and m == k
    # every nibble in turn: two values that first differ in nibble p
    for p in range(8):
        a = np.uint32(0x3A555555) & ~np.uint32(0xF << (28 - 4 * p)) | np.uint32((2 if p else 1) << (28 - 4 * p))
        b = a + np.uint32(1 << (28 - 4 * p))
        d2 = from_bits([b, a, b, a, a])
        assert (d2 <= R0SQ).all() and a < b
        assert check(evplp, d2, 3, rminsq=F(2.0 ** -140), what=f"nibble {p}") == (from_bits([a])[0], 3)
        assert check(evplp, d2, 4, rminsq=F(2.0 ** -140), what=f"nibble {p}") == (from_bits([b])[0], 5)


def test_zeros_denormals_and_values_that_are_no_candidates(evplp):
    tiny = F(2.0 ** -140)
    d2 = np.asarray([0.0, 0.0, 1e-45, 3e-42, 2.0 ** -126, 0.001, 0.3, np.inf, 1e30, float(np.nextafter(R0SQ, F(1))), float(R0SQ)], F)
    assert check(evplp, d2, 1, rminsq=tiny, what="zero, floored") == (tiny, 3)        # 0, 0 and 1e-45 lie within 2^-140
    assert check(evplp, d2, 3, rminsq=F(1e-45), what="the smallest denormal")[0] == F(1e-45)
    assert check(evplp, d2, 4, rminsq=tiny, what="a denormal") == (F(3e-42), 4)
    assert check(evplp, d2, 5, rminsq=tiny, what="the smallest normal") == (F(2.0 ** -126), 5)
    assert check(evplp, d2, 7, rminsq=tiny, what="r0sq itself is a candidate") == (R0SQ, 7)
    assert check(evplp, d2, 8, rminsq=tiny, what="what lies above r0sq is not") == (R0SQ, 7)
    only_far = np.asarray([0.3, 0.26, np.inf], F)
    assert check(evplp, only_far, 1, what="no candidate at all") == (R0SQ, 0)


def test_both_clamps(evplp):
    d2 = np.asarray([1e-6, 2e-6, 3e-6, 0.01, 0.02, 0.25], F)
    rmin = F(2.5e-6)
    assert check(evplp, d2, 1, rminsq=rmin, what="floor") == (rmin, 2)
    assert check(evplp, d2, 2, rminsq=rmin, what="floor") == (rmin, 2)
    assert check(evplp, d2, 3, rminsq=rmin, what="just above the floor") == (F(3e-6), 3)
    assert check(evplp, d2, 3, rminsq=F(3e-6), what="the floor is the k-th") == (F(3e-6), 3)
    assert check(evplp, d2, 6, rminsq=rmin, what="the ceiling is the k-th") == (R0SQ, 6)
    assert check(evplp, d2, 7, rminsq=rmin, what="the ceiling for want of candidates") == (R0SQ, 6)
    assert check(evplp, d2, 2, rminsq=R0SQ, what="floor == ceiling") == (R0SQ, 6)
    # a floor between two neighbouring floats' prefixes: the early exit of the select must not take a k-th above the floor for one below
    lad = ladder(0.0123, 64)
    for f in (lad[0], lad[15], lad[16], lad[17], lad[63]):
        for k in (1, 16, 17, 18, 64):
            check(evplp, lad, k, rminsq=f, what="floor inside a ladder")


@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 257, 1000, 4999, 5000])
def test_random_sets(evplp, n):
    rng = np.random.RandomState(n)
    kinds = [(rng.rand(n) * 0.3).astype(F),                                                    # some above r0sq
             (rng.rand(n) ** 8 * 0.25).astype(F),                                               # crowded towards 0
             (F(0.01) + (rng.randint(0, 7, n) * F(2.0 ** -30)).astype(F)).astype(F),           # seven values, many ties
             from_bits(rng.randint(0, 0x3E800000, n).astype(np.uint32))]                        # every exponent, denormals included
    for d2 in kinds:
        C_ = int((~(d2 > R0SQ)).sum())
        for k in sorted({1, 2, max(1, C_ // 2), max(1, C_ - 1), max(1, C_), C_ + 1, n + 1}):
            check(evplp, d2, k, rminsq=F(2.0 ** -100), what=f"random {n}")
            check(evplp, d2, k, rminsq=F(1e-3), what=f"random {n}, floored")


def test_the_select_refuses(evplp):
    L = evplp.lib()
    d2 = np.asarray([0.1, 0.2], F)
    r, m = C.c_float(7.0), C.c_uint32(7)
    p = d2.ctypes.data_as(C.c_void_p)

    def call(ptr=p, n=2, k=1, rminsq=1e-6, r0sq=0.25, out=C.byref(r), outm=C.byref(m)):
        return L.evplp_knn_radius2(ptr, n, k, rminsq, r0sq, out, outm)
    assert call() == evplp.OK and r.value == F(0.1) and m.value == 1
    r.value, m.value = 7.0, 7
    INV = evplp.ERR_INVALID
    assert call(k=0) == INV and call(ptr=None) == INV and call(out=None) == INV and call(outm=None) == INV
    assert call(rminsq=0.0) == INV and call(rminsq=-1.0) == INV and call(rminsq=0.3) == INV and call(rminsq=float("nan")) == INV and call(r0sq=float("inf")) == INV
    for bad in (np.nan, -0.0, -1.0):
        b = np.asarray([0.1, bad], F)
        assert call(ptr=b.ctypes.data_as(C.c_void_p)) == INV, bad
    assert r.value == 7.0 and m.value == 7, "a refused call writes nothing"
    assert call(ptr=None, n=0) == evplp.OK and r.value == 0.25 and m.value == 0


# ---------------------------------------------------------------------------------------------------------------- the seed
def restate_seed(state, radius2, m, phi, alpha):
    """include/evplp.h's first photon half in numpy float32 scalars: every operation rounded to fp32 on its own, IEEE division"""
    s = state.copy()
    alpha, phi = F(alpha), np.asarray(phi, F)
    s["radius2"][0] = F(radius2)
    if m > 0:
        mf = F(m)
        n = s["n"][0]
        nn = F(n + F(alpha * mf))
        ratio = F(nn / F(n + mf))
        s["radius2"][0] = F(s["radius2"][0] * ratio)
        for k in range(3):
            s["tau"][0, k] = F(F(s["tau"][0, k] + phi[k]) * ratio)
        s["n"][0] = nn
    s["pm_calls"] = 1
    return s


def state_of(evplp, **kw):
    s = np.zeros(1, evplp.SURFACE_STATE_DTYPE)
    for k, v in kw.items():
        s[k][0] = v
    return s


# (name, the state's fields, radius2, M, phi, alpha, r0sq)
SEEDS = [
    ("fresh", {}, 0.0123, 8, (0.25, 0.5, 0.125), 2.0 / 3.0, 0.09),
    ("fresh, M = 0: the radius and the count alone", {}, 0.09, 0, (0.0, 0.0, 0.0), 2.0 / 3.0, 0.09),
    ("fresh, M = 1", {}, 1e-7, 1, (0.3, 0.2, 0.1), 0.7, 0.0123),
    ("alpha = 1: radius2 keeps its bits", {}, 0.0131, 17, (0.1, 0.2, 0.3), 1.0, 0.02),
    ("after a VPL half: its sums stay", dict(vpl=(1, 2, 3), lit_sum=5, vpl_calls=2), 0.004, 64, (3.0, 2.0, 1.0), 2.0 / 3.0, 0.01),
    ("garbage radius2 before the first photon half", dict(radius2=float("nan"), vpl=(1, 2, 3), lit_sum=5, vpl_calls=1), 0.004, 2, (0.1, 0.2, 0.3), 0.5, 0.09),
    ("radius2 at the smallest the call admits", {}, 2.0 ** -100, 3, (1e-5, 2e-5, 3e-5), 0.1, 0.01),
    ("radius2 denormal", {}, float(F(3e-42)), 2, (1e-5, 2e-5, 3e-5), 2.0 / 3.0, 0.01),
    ("radius2 equals r0sq", {}, float(F(0.09)), 4, (0.1, 0.2, 0.3), 0.5, float(F(0.09))),
    ("many photons", {}, 0.003, 100000, (31.0, 32.0, 33.0), 2.0 / 3.0, 0.01),
    ("n and tau that are not zero are used as they are", dict(tau=(0.5, 0.25, 0.125), n=3.5), 0.003, 5, (1.0, 2.0, 3.0), 2.0 / 3.0, 0.01),
]


@pytest.mark.parametrize("case", SEEDS, ids=[c[0] for c in SEEDS])
def test_the_seed_matches_the_float32_restatement_bit_for_bit(evplp, case):
    name, fields, radius2, m, phi, alpha, r0sq = case
    before = state_of(evplp, **fields)
    got = evplp.surface_state_seed(before, radius2, m, phi, alpha, r0sq)
    want = restate_seed(before, radius2, m, phi, alpha)
    assert got.tobytes() == want.tobytes(), (name, got, want)
    assert got["pm_calls"][0] == 1 and got["flags"][0] == 0
    assert got["vpl"].tobytes() == before["vpl"].tobytes() and got["lit_sum"][0] == before["lit_sum"][0] and got["vpl_calls"][0] == before["vpl_calls"][0]
    assert got["radius2"][0] <= F(radius2) and (m == 0 or alpha < 1.0 or bits(got["radius2"])[0] == bits(F(radius2))[()])
    if m == 0:
        assert got["tau"].tobytes() == before["tau"].tobytes() and got["n"].tobytes() == before["n"].tobytes()
    # seeded at r0sq, a state is the progressive call's first photon half
    if F(radius2) == F(r0sq):
        assert got.tobytes() == evplp.surface_state_update(before, m, phi, alpha, r0sq).tobytes()
    # ... and what follows is an ordinary state: one more update goes through, the resolve divides by the shrunken radius
    nxt = evplp.surface_state_update(got, 3, (0.1, 0.1, 0.1), alpha, r0sq)
    assert nxt["flags"][0] == 0 and nxt["pm_calls"][0] == 2 and nxt["radius2"][0] <= got["radius2"][0]


def test_the_seed_refuses_a_state_that_is_not_fresh(evplp):
    L = evplp.lib()
    phi = np.asarray([0.1, 0.2, 0.3], F)
    pp = phi.ctypes.data_as(C.c_void_p)
    for fields in (dict(pm_calls=1, radius2=0.01, n=2.0), dict(pm_calls=7, radius2=0.01), dict(flags=1), dict(flags=1, vpl_calls=3)):
        s = state_of(evplp, **fields)
        keep = s.tobytes()
        assert L.evplp_surface_state_seed(s.ctypes.data_as(C.c_void_p), 0.01, 4, pp, 0.5, 0.09) == evplp.ERR_INVALID, fields
        assert s.tobytes() == keep, "not a byte is touched"
        with pytest.raises(ValueError):
            evplp.surface_state_seed(s, 0.01, 4, phi, 0.5, 0.09)
    s = state_of(evplp)
    for bad in (0.0, -0.01, float("nan"), float("inf"), float(np.nextafter(F(0.09), F(1)))):
        assert L.evplp_surface_state_seed(s.ctypes.data_as(C.c_void_p), bad, 4, pp, 0.5, float(F(0.09))) == evplp.ERR_INVALID, bad
    assert L.evplp_surface_state_seed(None, 0.01, 4, pp, 0.5, 0.09) == evplp.ERR_INVALID and L.evplp_surface_state_seed(s.ctypes.data_as(C.c_void_p), 0.01, 4, None, 0.5, 0.09) == evplp.ERR_INVALID
    assert s.tobytes() == bytes(48)


def test_fresh_seed_resolve_is_the_k_nearest_density_estimate(evplp):
    """alpha = 1: ratio is exactly 1, so pm = (Phi InvPi) / rk2"""
    inv_pi = F(0.318309886183790671537767526745028724068919291480912897495)
    phi = np.asarray([0.75, 1.5, 0.375], F)
    rk2 = F(0.0037)
    s = evplp.surface_state_seed(np.zeros(1, evplp.SURFACE_STATE_DTYPE), rk2, 8, phi, 1.0, 0.01)
    r = evplp.surface_state_resolve(s)
    assert r["pm"][0].tobytes() == np.asarray([F(F(p * inv_pi) / rk2) for p in phi], F).tobytes() and r["photons"][0] == 8.0
