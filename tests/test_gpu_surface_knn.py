"""k-nearest-photon start radii on the device (evplp_gather_surface_knn, evplp_bake_lightmap_knn_device), on test_gpu_surface.py's sizes --
scenes.box_room, the oracle's 64 x 48 G-buffer as 3 072 points, 2 000 x 4 record slots; the records are the oracle's light paths of four
seeds -- against a numpy brute force over ALL photons: d2 of every (photon, point) pair in float32 with the fragment's roundings, the
candidates !(d2 > r0sq), the k-th smallest by np.sort, the clamp, the photons inside the selected radius.

  1  radius and estimate, modes 0 / 4 / 5, alpha = 1 (ratio is exactly 1: radius2 holds rk2's bits), k = 1 at r0 = 1 x the room's radius
     and k = 8 at r0 = 2 x.  The multiples were chosen on the CPU, with the oracle's records, so that both branches are well filled; of the
     3 040 valid points, k = 1: 2 588 have C >= 1 (85.1 %), 452 have C = 0 (14.9 %); k = 8: 1 720 have C >= 8 (56.6 %), 1 320 have C < 8
     (43.4 %) -- the test asserts at least 40 % and at least 5 %.  radius2 and n bit for bit, tau against the float64 fragment of
     tests/shading_domain.py under the bar test_gpu_surface_progressive.py builds for one iteration (K_GPU_SPLAT).
  2  k above every C: the progressive call's bytes.   3  seed, then three progressive iterations, restated.
  4  hostile sets in one wave and one lane of the next, and 5 000 photons in one cell.
  5  a point's 48 bytes.   6  refusals.   7  the 32 x 32 atlas at S = 2.

Measured on an MI355X, 2026-10-21 (`pytest -s -m gpu tests/test_gpu_surface_knn.py` prints them).  k = 1: 2 588 photons inside the selected
radii, 25 points at the floor, tau error / bar at its worst 0.108 / 0.224 / 0.140 in modes 0 / 4 / 5; k = 8: 20 417 photons, 0.119 / 0.219 /
0.135 (K = 18); no undecided fragment.  Seeded at k = 8, then three iterations at alpha = 2/3: M 14 325, 11 864, 10 436, mean radius2 /
r0sq 0.374.  Hostile sets: C 0 .. 9, M 0 .. 4, five different radii, tau error / bar 0.117.  5 000 photons in one cell: 27, 19, 9 and 0
of 48 points select at k = 1, 2 500, 5 000, 5 001.  Lightmap: 2 293 covered samples, 786 with k photons or more, mean radius2 / r0sq 0.639.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import shading_domain as sd
from test_gpu_lightmap import band, bits, packed_uvs
from test_gpu_shading_domain import K_GPU_SPLAT
from test_gpu_surface import NPATHS, P, Room, dot32, floor_box, floor_points, hostile_records, room_context
from test_gpu_surface_progressive import inside_own, phi_f64, restate, usable_photons

pytestmark = pytest.mark.gpu

F = np.float32
MODES = (0, 4, 5)
SEEDS = (5, 6, 7, 8)
ALPHA = 2.0 / 3.0
R0_MULT = {1: 1.0, 8: 2.0}          # k -> r0 as a multiple of the room's radius (the docstring gives the counts)
INV_PI = F(0.318309886183790671537767526745028724068919291480912897495)


def say(*a):
    print("[surface knn]", *a, flush=True)


# ---------------------------------------------------------------------------------------------------------------- the brute force
def brute(rec, slots, X, r0sq, k, rminsq, live):
    """include/evplp.h's definitions over all usable photons: per point C, rk2, the [photons, points] matrix of the photons inside rk2, M,
    and the photons' slots"""
    ph = usable_photons(rec, slots)
    r0sq, rminsq = F(r0sq), F(rminsq)
    with np.errstate(all="ignore"):
        dv = rec["pos"][ph][:, None, :].astype(F) - X[None, :, :].astype(F)
        d2 = dot32(dv, dv)
        cand = ~(d2 > r0sq) & live[None, :]
        C_ = cand.sum(0)
        if k <= len(ph):
            kth = np.sort(np.where(cand, d2, F(np.inf)), axis=0)[k - 1]
        else:
            kth = np.full(len(X), np.inf, F)
        kth = np.where(C_ >= k, kth, r0sq).astype(F)
        rk2 = np.minimum(np.maximum(kth, rminsq), r0sq).astype(F)
        inside = cand & ~(d2 > rk2[None, :])
    return SimpleNamespace(C=C_, rk2=rk2, inside=inside, M=inside.sum(0), slots=ph, kth=kth)


def seed_restated(state, rk2, M, alpha, live):
    """the first photon half of include/evplp.h over arrays, every operation a float32 one; tau is left alone.  The new state and the ratio."""
    s = state.copy()
    alpha = F(alpha)
    s["radius2"] = np.where(live, rk2, s["radius2"]).astype(F)
    hit = live & (M > 0)
    m = M.astype(F)
    with np.errstate(all="ignore"):
        nn = s["n"] + alpha * m
        ratio = np.where(hit, nn / (s["n"] + m), F(1)).astype(F)
    s["radius2"] = np.where(hit, s["radius2"] * ratio, s["radius2"])
    s["n"] = np.where(hit, nn, s["n"])
    s["pm_calls"] = np.where(live, 1, s["pm_calls"]).astype(np.uint32)
    return s, ratio


# ---------------------------------------------------------------------------------------------------------------- the room, once
@pytest.fixture(scope="module")
def prog(evplp, oracle):
    room = Room(evplp)
    room.recs = [room.osc.trace_light_paths(s, NPATHS, P) for s in SEEDS]
    room.pts["valid"][5::97] = 0.0                  # (the room is closed: every pixel shows a surface) stencilled points among them
    room.valid = room.pts["valid"] != 0
    assert room.valid.sum() > 0.9 * room.n and not room.valid.all()
    room.found = {}
    for k, mult in R0_MULT.items():
        r0 = float(F(mult * room.radius))
        r0sq = F(r0) * F(r0)
        rmin = float(F(r0 / 16.0))
        room.found[k] = SimpleNamespace(r0=r0, r0sq=r0sq, rmin=rmin, rminsq=F(rmin) * F(rmin),
                                        b=brute(room.recs[0], NPATHS * P, room.pts["pos"], r0sq, k, F(rmin) * F(rmin), room.valid))
    return room


def params(room, mode, r0):
    p = room.params(mode)
    p["photon_radius"] = r0
    return p


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("k", sorted(R0_MULT))
@pytest.mark.parametrize("mode", MODES)
def test_radius_and_estimate_against_the_brute_force(evplp, prog, mode, k):
    f = prog.found[k]
    b, v = f.b, prog.valid
    enough, few = int((b.C[v] >= k).sum()), int((b.C[v] < k).sum())
    say(f"k = {k}, r0 = {R0_MULT[k]} x the room's radius: of {int(v.sum())} valid points {enough} have C >= k, {few} have C < k; {int((b.rk2[v] == f.rminsq).sum())} at the floor")
    assert enough >= 0.4 * v.sum() and few >= 0.05 * v.sum()
    fpd = params(prog, mode, f.r0)
    with room_context(evplp, prog, prog.recs[0]) as c:
        got = c.gather_surface_knn(prog.pts, evplp.frame_params(**fpd), np.zeros(prog.n, evplp.SURFACE_STATE_DTYPE), k, f.rmin, alpha=1.0)
        res = c.surface_resolve(got)
    assert got[~v].tobytes() == bytes(48 * int((~v).sum())), "a stencilled point's state stays fresh"
    assert (got["flags"] == 0).all() and (got["pm_calls"][v] == 1).all() and (got["vpl_calls"] == 0).all()
    assert (got["vpl"] == 0).all() and (got["lit_sum"] == 0).all()
    assert np.array_equal(bits(got["radius2"][v]), bits(b.rk2[v])), np.nonzero(v & (bits(got["radius2"]) != bits(b.rk2)))[0][:8]
    assert np.array_equal(bits(got["n"][v]), bits(b.M[v].astype(F))), np.nonzero(v & (got["n"] != b.M))[0][:8]
    sel = v & (b.C >= k)
    assert (b.M[sel] >= k).all() and (got["radius2"][sel] <= f.r0sq).all() and (got["radius2"][v & (b.C < k)] == f.r0sq).all()
    phi, pbar, dec = phi_f64(mode, fpd, prog.pts, prog.recs[0], b.inside, b.slots)
    tbar = pbar + 2.0 * 2.0 ** -24 * np.abs(phi)
    ok = dec & v
    err = np.abs(got["tau"].astype(np.float64) - phi)
    worst = float((err[ok] / (tbar[ok] + 1e-20)).max())
    say(f"k = {k}, mode {mode}: {int(b.M.sum())} photons inside the selected radii, tau error / bar at its worst {worst:.3f} (K = {K_GPU_SPLAT}), {int((~dec & v).sum())} points with an undecided fragment")
    assert np.isfinite(got["tau"]).all() and worst <= 1.0 and dec[v].mean() > 0.9 and (got["tau"][~v] == 0).all()
    # fresh states + this call + the resolve: the k-nearest density estimate Phi InvPi / rk2, and photons = M
    with np.errstate(all="ignore"):
        want = ((got["tau"] * INV_PI) / (got["radius2"] * F(1))[:, None]).astype(F)
    assert np.array_equal(bits(res["pm"][v]), bits(want[v])) and np.array_equal(res["photons"][v], got["n"][v]) and np.abs(res["pm"]).max() > 1e-4


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("mode", MODES)
def test_k_above_every_count_is_the_progressive_call(evplp, prog, mode):
    fpd = prog.params(mode)
    fp = evplp.frame_params(**fpd)
    fresh = np.zeros(prog.n, evplp.SURFACE_STATE_DTYPE)
    with room_context(evplp, prog, prog.recs[0]) as c:
        want = c.gather_surface_progressive(prog.pts, fp, fresh, alpha=ALPHA, what=evplp.SURFACE_PHOTONS)
        got = c.gather_surface_knn(prog.pts, fp, fresh, 2 ** 24, prog.radius / 8.0, alpha=ALPHA)
    assert want["n"].sum() > 3000 and (want["pm_calls"][prog.valid] == 1).all()
    assert got.tobytes() == want.tobytes(), np.nonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])[0][:8]


# ---------------------------------------------------------------------------------------------------------------- 3
def test_seed_then_three_progressive_iterations(evplp, prog):
    mode, k = 5, 8
    f = prog.found[k]
    v = prog.valid
    fp = evplp.frame_params(**params(prog, mode, f.r0))
    fresh = np.zeros(prog.n, evplp.SURFACE_STATE_DTYPE)
    want, _ = seed_restated(fresh, f.b.rk2, f.b.M, ALPHA, v)
    with room_context(evplp, prog, prog.recs[0]) as c:
        st = c.gather_surface_knn(prog.pts, fp, fresh, k, f.rmin, alpha=ALPHA)
        assert np.array_equal(bits(st["n"]), bits(want["n"])) and np.array_equal(bits(st["radius2"]), bits(want["radius2"])) and np.array_equal(st["pm_calls"], want["pm_calls"])
        assert (st["radius2"][v & (f.b.M > 0)] < f.b.rk2[v & (f.b.M > 0)]).all() and (st["radius2"][v] > 0).all()
        counts = []
        for it, rec in enumerate(prog.recs[1:]):
            inside, _ = inside_own(rec, NPATHS * P, prog.pts["pos"], want["radius2"])
            inside &= v[None, :]
            M = inside.sum(0)
            before = want
            want, _ = restate(before, M, ALPHA, f.r0sq, v)
            c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
            st = c.gather_surface_progressive(prog.pts, fp, st, alpha=ALPHA, what=evplp.SURFACE_PHOTONS)
            grown = (st["n"].astype(np.float64) - before["n"].astype(np.float64)) / float(F(ALPHA))
            assert np.array_equal(np.rint(grown).astype(np.int64), M), (it, np.nonzero(np.rint(grown) != M)[0][:8])
            assert np.array_equal(bits(st["n"]), bits(want["n"])) and np.array_equal(bits(st["radius2"]), bits(want["radius2"])), it
            assert (st["flags"] == 0).all() and (st["pm_calls"][v] == it + 2).all() and (st["pm_calls"][~v] == 0).all()
            counts.append(int(M.sum()))
    say(f"seeded at k = {k}, then three iterations at alpha = 2/3: M per iteration {counts}; mean radius2 / r0sq {float(st['radius2'][v].mean() / f.r0sq):.3f}")
    assert min(counts) > 1000


# ---------------------------------------------------------------------------------------------------------------- 4
def test_hostile_sets_in_one_wave_and_one_lane_of_the_next(evplp, oracle):
    """65 points on the line y = 0 of the floor, 0.28 apart, each with a photon set of its own within r0 = 0.125 at (x, +-d, 0), so that
    dv = (0, +-d, 0) and d2 = fl(d d) exactly.  k = 4."""
    scene = sd.floor_scene()
    lo, hi = floor_box(scene)
    n, k = 65, 4
    r0 = 0.125
    r0sq = F(r0) * F(r0)
    rmin = float(F(2.0 ** -12))
    rminsq = F(rmin) * F(rmin)
    up = F(np.inf)
    X = np.zeros((n, 3), F); X[:, 0] = (-10.0 + 0.28 * np.arange(n)).astype(F)
    assert X[:, 0].max() < hi[0] and X[:, 0].min() > lo[0]
    kinds = ["tie_k", "few", "tie_below", "on_point", "ulp", "denormal", "stencil", "at_r0", "used", "vpl_only", "flagged", "none", "floor_mix"]
    kind = [kinds[i % len(kinds)] for i in range(n)]
    kind[20] = "nan_point"; kind[33] = "inf_eye"; kind[40] = "outside_near"; kind[41] = "outside_far"; kind[64] = "ulp"
    st = np.zeros(n, evplp.SURFACE_STATE_DTYPE)
    pts = floor_points(evplp, X)
    eyes = np.ascontiguousarray(np.broadcast_to(np.asarray(sd.CAMERA, F), (n, 3))).copy()
    photons = []

    def put(i, ds):
        for j, d in enumerate(ds):
            photons.append([X[i, 0], F(d) if j % 2 == 0 else -F(d), 0.0])
    d1, d2_ = F(0.03125), F(0.046875)
    far = [F(0.09), F(0.1), F(0.11)]
    for i, kd in enumerate(kind):
        if kd == "tie_k":                   # k photons at one distance, three farther
            put(i, [d1] * k + far)
        elif kd == "few":                   # C = 2 < k
            put(i, [d1, d2_])
        elif kd == "tie_below":             # k - 1 tied below the k-th
            put(i, [d1] * (k - 1) + [d2_] + far)
        elif kd == "on_point":              # d2 = 0, k times: the floor
            put(i, [F(0)] * k + far)
        elif kd == "ulp":                   # distances one ulp apart
            lad = (bits(np.asarray([d1], F))[0] + np.arange(9, dtype=np.uint32)).view(F)
            put(i, list(lad[::-1]))
        elif kd == "denormal":              # d2 = 2^-140
            put(i, [F(2.0 ** -70)] * k + far)
        elif kd == "at_r0":                 # the k-th lies on r0 itself, one more an ulp beyond
            put(i, [d1] * (k - 1) + [F(r0), np.nextafter(F(r0), up), np.nextafter(F(r0), up)])
        elif kd == "floor_mix":             # two below the floor, the k-th above it
            put(i, [F(2.0 ** -13), F(2.0 ** -14), d1, d2_, F(0.05)])
        elif kd in ("stencil", "used", "vpl_only", "flagged", "nan_point", "inf_eye"):
            put(i, [d1] * k + far)
        if kd == "stencil":
            pts["valid"][i] = 0.0
            st[i:i + 1].view(np.uint8)[:] = 0xA5
        if kd == "used":
            st[i] = ((0.5, 0.25, 0.125), r0sq * F(0.5), (1.0, 2.0, 3.0), 6.0, 4.0, 2, 1, 0)
        if kd == "flagged":
            st[i] = ((0.5, 0.25, 0.125), 0.0, (1.0, 2.0, 3.0), 6.0, 4.0, 2, 0, 1)
        if kd == "vpl_only":
            st[i] = ((0.0, 0.0, 0.0), 0.0, (1.0, 2.0, 3.0), 0.0, 4.0, 2, 0, 0)
        if kd == "nan_point":
            pts["pos"][i, 2] = np.nan
        if kd == "inf_eye":
            eyes[i, 0] = np.inf
    X[40] = (float(lo[0]) - 0.05, 0.0, 0.0); X[41] = (1.0e6, 0.0, 0.0)
    pts["pos"][40] = X[40]; pts["pos"][41] = X[41]
    photons = np.asarray(photons, F)
    rec = hostile_records(photons)
    slots = 2 * len(photons)
    kd = np.asarray(kind)
    flagged_now = np.isin(kd, ("nan_point", "inf_eye"))
    untouched = np.isin(kd, ("stencil", "used", "flagged"))
    live = ~flagged_now & ~untouched
    b = brute(rec, slots, X, r0sq, k, rminsq, live)
    want, ratio = seed_restated(st, b.rk2, b.M, ALPHA, live)
    # the sets do what they were built for
    assert (b.C[kd == "few"] == 2).all() and (b.rk2[kd == "few"] == r0sq).all() and (b.C[np.isin(kd, ("none", "outside_near", "outside_far"))] == 0).all()
    assert (b.rk2[kd == "tie_k"] == d1 * d1).all() and (b.M[kd == "tie_k"] == k).all()
    assert (b.rk2[kd == "tie_below"] == d2_ * d2_).all() and (b.M[kd == "tie_below"] == k).all()
    assert (b.rk2[np.isin(kd, ("on_point", "denormal"))] == rminsq).all() and (b.M[np.isin(kd, ("on_point", "denormal"))] == k).all()
    assert (b.kth[kd == "denormal"] == F(2.0 ** -140)).all() and (b.kth[kd == "on_point"] == 0).all()
    assert (b.rk2[kd == "at_r0"] == r0sq).all() and (b.C[kd == "at_r0"] == k).all()
    assert (b.rk2[kd == "floor_mix"] == d2_ * d2_).all() and (b.M[kd == "ulp"] >= k).all() and len(np.unique(bits(b.rk2[live]))) >= 5
    mode = 5
    kw = dict(camera_pos=sd.CAMERA, mis_mode=mode, pdf_mc=0.02, clamping_value=0.02, photon_radius=r0, num_light_paths=len(photons), num_vpl_light_paths=1, photons_per_path=2)
    with evplp.Context(sd.W, sd.H, len(photons), 1, 2, deterministic=True) as c:
        scene.upload(c)
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        got = c.gather_surface_knn(pts, evplp.frame_params(**kw), st, k, rmin, alpha=ALPHA, eyes=eyes)
    assert got[untouched].tobytes() == st[untouched].tobytes(), "stencilled, used and flagged states keep all 48 bytes"
    keep = st[flagged_now].copy(); keep["flags"] |= 1
    assert got[flagged_now].tobytes() == keep.tobytes(), "a point or eye that is not finite: flagged, every other byte kept"
    assert np.array_equal(bits(got["radius2"][live]), bits(want["radius2"][live])), np.nonzero(live & (bits(got["radius2"]) != bits(want["radius2"])))[0]
    assert np.array_equal(bits(got["n"][live]), bits(want["n"][live])), np.nonzero(live & (bits(got["n"]) != bits(want["n"])))[0]
    assert (got["pm_calls"][live] == 1).all() and (got["flags"][live] == 0).all()
    for name in ("vpl", "lit_sum", "vpl_calls"):
        assert got[name][live].tobytes() == st[name][live].tobytes(), name
    empty = live & (b.M == 0)
    assert empty.sum() >= 3 and (bits(got["radius2"][empty]) == bits(np.asarray([r0sq]))[0]).all() and (got["n"][empty] == 0).all() and (got["tau"][empty] == 0).all()
    phi, pbar, dec = phi_f64(mode, kw, pts, rec, b.inside, b.slots)
    r64 = ratio.astype(np.float64)[:, None]
    tau = (st["tau"].astype(np.float64) + phi) * r64
    tbar = pbar * r64 + 3.0 * 2.0 ** -24 * np.abs(tau) + 1e-20
    ok = live & dec
    worst = float((np.abs(got["tau"].astype(np.float64) - tau)[ok] / tbar[ok]).max())
    say(f"hostile sets: C {b.C[live].min()} .. {b.C[live].max()}, M {b.M[live].min()} .. {b.M[live].max()}, {len(np.unique(bits(b.rk2[live])))} different radii, tau error / bar at its worst {worst:.3f}")
    assert ok.sum() > 30 and worst <= 1.0


def test_five_thousand_photons_in_one_cell(evplp, oracle):
    """the crowd of test_gpu_surface.py's hostile grid, drawn together so that the points in its middle have all of it within r0:
    k = 1, 2 500, 5 000 and 5 001 over the same 48 points"""
    scene = sd.floor_scene()
    lo, hi = floor_box(scene)
    rng = np.random.RandomState(19)
    r0 = 0.25
    r0sq = F(r0) * F(r0)
    rmin = float(F(2.0 ** -10))
    rminsq = F(rmin) * F(rmin)
    n_cell = 5000
    edge, gbits = evplp.photon_grid_plan(r0, lo, hi, 2 * n_cell)
    cell0 = lo[:2].astype(np.float64) + np.array([30.0, 12.0]) * float(edge)
    crowd = np.zeros((n_cell, 3), F)
    crowd[:, :2] = (cell0 + rng.uniform(0.25, 0.75, (n_cell, 2)) * float(edge)).astype(F)
    cells = np.stack([evplp.photon_grid_cell(p, lo, edge, gbits)[0] for p in crowd[::50]])
    assert len(np.unique(cells, axis=0)) == 1, "one cell"
    X = np.zeros((48, 3), F)
    X[:8, :2] = (cell0 + rng.uniform(0.45, 0.55, (8, 2)) * float(edge)).astype(F)          # the middle: the whole crowd within r0
    X[8:, :2] = (cell0 + rng.uniform(-0.6, 1.6, (40, 2)) * float(edge)).astype(F)          # in and around it
    X[8, :2] = crowd[17, :2]                                                                # on a photon
    pts = floor_points(evplp, X)
    rec = hostile_records(crowd)
    live = np.ones(len(X), bool)
    fresh = np.zeros(len(X), evplp.SURFACE_STATE_DTYPE)
    kw = dict(camera_pos=sd.CAMERA, mis_mode=0, pdf_mc=0.02, clamping_value=0.02, photon_radius=r0, num_light_paths=n_cell, num_vpl_light_paths=1, photons_per_path=2)
    with evplp.Context(sd.W, sd.H, n_cell, 1, 2, deterministic=True) as c:
        scene.upload(c)
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        for k in (1, 2500, 5000, 5001):
            b = brute(rec, 2 * n_cell, X, r0sq, k, rminsq, live)
            want, _ = seed_restated(fresh, b.rk2, b.M, ALPHA, live)
            got = c.gather_surface_knn(pts, evplp.frame_params(**kw), fresh, k, rmin, alpha=ALPHA)
            assert np.array_equal(bits(got["radius2"]), bits(want["radius2"])), (k, np.nonzero(bits(got["radius2"]) != bits(want["radius2"]))[0])
            assert np.array_equal(bits(got["n"]), bits(want["n"])), (k, np.nonzero(bits(got["n"]) != bits(want["n"]))[0])
            assert (got["pm_calls"] == 1).all() and (got["flags"] == 0).all() and np.isfinite(got["tau"]).all()
            say(f"5 000 photons in one cell, k = {k}: C {b.C.min()} .. {b.C.max()}, {int((b.C >= k).sum())} of {len(X)} points select, M {b.M.min()} .. {b.M.max()}")
            assert (b.C[:8] == n_cell).all() and b.C.min() < 2500 and b.rk2[8] == (rminsq if k == 1 else b.rk2[8])
            assert ((b.C >= k).sum() >= 8) == (k <= n_cell) and ((b.C >= k).sum() == 0) == (k > n_cell)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_points_48_bytes_do_not_depend_on_the_batch_the_form_or_the_buckets(evplp, prog, monkeypatch):
    import torch
    mode, k = 5, 8
    f = prog.found[k]
    fp = evplp.frame_params(**params(prog, mode, f.r0))
    # states of three kinds: fresh ones, ones a VPL half has been through, ones a photon half has been through (those stay as they are)
    states = np.zeros(prog.n, evplp.SURFACE_STATE_DTYPE)
    states["vpl"][1::3] = (0.25, 0.5, 0.75); states["lit_sum"][1::3] = 3.0; states["vpl_calls"][1::3] = 2
    used = np.zeros(prog.n, bool); used[2::7] = True
    states["radius2"][used] = f.r0sq * F(0.25); states["n"][used] = 5.0; states["tau"][used] = (0.1, 0.2, 0.3); states["pm_calls"][used] = 3

    def run(c, pts, st):
        return c.gather_surface_knn(pts, fp, st, k, f.rmin, alpha=ALPHA)
    n = evplp.SURFACE_CHUNK + 65
    src = (np.arange(n) * 7 + 3) % prog.n
    with room_context(evplp, prog, prog.recs[0]) as c:
        base = run(c, prog.pts, states)
        assert base[used].tobytes() == states[used].tobytes() and len(np.unique(bits(base["radius2"][prog.valid & ~used]))) > 200
        assert run(c, prog.pts, states).tobytes() == base.tobytes(), "two runs"
        for i in (0, 1, 2, 777, prog.n - 1):
            assert run(c, prog.pts[i:i + 1], states[i:i + 1]).tobytes() == base[i:i + 1].tobytes(), i
        big = run(c, prog.pts[src], states[src])
        assert big.tobytes() == base[src].tobytes(), np.nonzero([g.tobytes() != x.tobytes() for g, x in zip(big, base[src])])[0][:8]
        # the device form, across the chunk boundary too
        d = torch.from_numpy(np.ascontiguousarray(prog.pts[src]).view(F).reshape(-1, 16)).cuda()
        s = torch.from_numpy(np.ascontiguousarray(states[src]).view(F).reshape(-1, 12).copy()).cuda()
        torch.cuda.synchronize()
        out = run(c, d, s)
        c.synchronize()
        assert out.data_ptr() == s.data_ptr() and out.cpu().numpy().tobytes() == base[src].tobytes(), "the device form"
    for grid_bits in ("1", "9"):                                        # two buckets; 512
        monkeypatch.setenv("EVPLP_SURFACE_GRID_BITS", grid_bits)
        with room_context(evplp, prog, prog.recs[0]) as c:
            assert run(c, prog.pts, states).tobytes() == base.tobytes(), f"EVPLP_SURFACE_GRID_BITS = {grid_bits}"


# ---------------------------------------------------------------------------------------------------------------- 6
def test_refusals_leave_the_states_and_the_context_untouched(evplp, prog):
    import torch
    L = evplp.lib()
    INV = evplp.ERR_INVALID
    pts = prog.pts[:8].copy()
    st = np.full(8 * 48, 0x5A, np.uint8)
    xp, sp = pts.ctypes.data, st.ctypes.data
    r0 = prog.radius

    def prm(**kw):
        p = prog.params(5); p.update(kw)
        return C.byref(evplp.frame_params(**p))

    def knn(k=8, r_min=r0 / 8.0, alpha=ALPHA, flags=0):
        return C.byref(evplp.KnnParams(k, r_min, alpha, flags))
    bad_knn = [dict(k=0), dict(flags=1), dict(flags=0x80000000)]
    bad_knn += [dict(r_min=x) for x in (0.0, -r0 / 8.0, float("nan"), float("inf"), float(np.nextafter(F(r0), F(np.inf))), 2.0 * r0, 1e-26, 2.0 ** -51)]
    bad_knn += [dict(alpha=x) for x in (0.0, -0.5, 1.0000001, float("nan"), float("inf"))]
    fresh = np.zeros(8, evplp.SURFACE_STATE_DTYPE)
    with room_context(evplp, prog, prog.recs[0]) as c:
        base = c.gather_surface_knn(pts, evplp.frame_params(**prog.params(5)), fresh, 8, r0 / 8.0, alpha=ALPHA)
        d = torch.from_numpy(pts.view(F).reshape(-1, 16)).cuda()
        o = torch.full((8 * 12 + 4,), 7.0, dtype=torch.float32, device="cuda")
        for form, px, ps in ((L.evplp_gather_surface_knn, xp, sp), (L.evplp_gather_surface_knn_device, C.c_void_p(d.data_ptr()), C.c_void_p(o.data_ptr()))):
            for mode in (1, 2, 3):
                assert form(c._h, prm(mis_mode=mode), knn(), px, None, 8, ps) == INV and b"pdf_mc" in L.evplp_last_error(c._h), mode
            assert form(c._h, prm(mis_mode=6), knn(), px, None, 8, ps) == INV
            for bad in bad_knn:
                assert form(c._h, prm(), knn(**bad), px, None, 8, ps) == INV, bad
            assert form(c._h, prm(), knn(k=0), px, None, 8, ps) == INV and b"k is 0" in L.evplp_last_error(c._h)
            assert form(c._h, prm(), knn(r_min=1e-26), px, None, 8, ps) == INV and b"r_min" in L.evplp_last_error(c._h)
            assert form(c._h, prm(), None, px, None, 8, ps) == INV and b"null params" in L.evplp_last_error(c._h)
            assert form(c._h, prm(), knn(), px, None, 8, None) == INV and form(c._h, prm(), knn(), None, None, 8, ps) == INV
            assert form(c._h, None, knn(), px, None, 8, ps) == INV and form(c._h, prm(), knn(), px, None, -1, ps) == INV
            assert form(c._h, prm(photon_radius=0.0), knn(), px, None, 8, ps) == INV and form(c._h, prm(num_light_paths=NPATHS + 1), knn(), px, None, 8, ps) == INV
            assert form(c._h, prm(), knn(k=0), px, None, 0, ps) == INV, "refused before n = 0 is looked at"
            assert form(c._h, prm(), knn(), px, None, 0, ps) == evplp.OK and form(c._h, prm(), knn(), None, None, 0, None) == evplp.OK
            assert form(c._h, prm(), knn(r_min=r0), px, None, 0, ps) == evplp.OK, "r_min = photon_radius is allowed"
        assert L.evplp_gather_surface_knn_device(c._h, prm(), knn(), C.c_void_p(d.data_ptr()), None, 8, C.c_void_p(o.data_ptr() + 4)) == INV
        assert b"states are not 16-byte aligned" in L.evplp_last_error(c._h)
        # the atlas form
        lm = evplp.LightmapParams(-1, 2, 2, 1, 0, 0)
        bake = L.evplp_bake_lightmap_knn_device
        so = C.c_void_p(o.data_ptr())
        for bad in bad_knn:
            assert bake(c._h, prm(), knn(**bad), C.byref(lm), None, so) == INV, bad
        assert bake(c._h, prm(), None, C.byref(lm), None, so) == INV and bake(c._h, prm(), knn(), None, None, so) == INV and bake(c._h, None, knn(), C.byref(lm), None, so) == INV
        assert bake(c._h, prm(mis_mode=2), knn(), C.byref(lm), None, so) == INV and bake(c._h, prm(), knn(), C.byref(lm), None, None) == INV
        assert bake(c._h, prm(), knn(), C.byref(evplp.LightmapParams(-1, 2, 2, 3, 0, 0)), None, so) == INV
        assert bake(c._h, prm(), knn(), C.byref(evplp.LightmapParams(-1, 2, 2, 1, 0, 2)), None, so) == INV
        assert bake(c._h, prm(), knn(), C.byref(lm), None, C.c_void_p(o.data_ptr() + 4)) == INV
        c.synchronize()
        assert (st == 0x5A).all() and (o.cpu().numpy() == 7.0).all(), "a refused call writes nothing"
        again = c.gather_surface_knn(pts, evplp.frame_params(**prog.params(5)), fresh, 8, r0 / 8.0, alpha=ALPHA)
        assert again.tobytes() == base.tobytes() and (again["pm_calls"][prog.valid[:8]] == 1).all(), "the context is usable afterwards"


# ---------------------------------------------------------------------------------------------------------------- 7
def test_lightmap_states_are_the_gathers_on_the_rasters_own_points(evplp, prog):
    import torch
    W = H = 32
    S = 2
    mode, k = 0, 8
    f = prog.found[k]
    uv = packed_uvs(prog.scene)
    fp = evplp.frame_params(**params(prog, mode, f.r0))
    n = W * H * S * S

    def run(c):
        st = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
        c.bake_lightmap_knn(fp, st, W, H, S, k=k, r_min=f.rmin, alpha=ALPHA, uvs=uv)
        c.synchronize()
        return st
    with room_context(evplp, prog, prog.recs[0]) as c:
        st = run(c)
        hits = c.lightmap_samples(W, H, S, uvs=uv).reshape(-1)
        pts = c.surface_points(hits)
        want = c.gather_surface_knn(pts, fp, np.zeros(n, evplp.SURFACE_STATE_DTYPE), k, f.rmin, alpha=ALPHA)
        tex = c.bake_lightmap_resolve(st, W, H, S, gutter=1)
        with band(W * S * S):                                           # one texel row per band
            st_rows = run(c)
        # ... and an ordinary progressive iteration takes the seeded atlas
        c.upload(evplp.BUF_RECORDS, prog.recs[1].astype(evplp.RECORD_DTYPE))
        after = c.bake_lightmap_progressive_device(fp, st.clone(), W, H, S, alpha=ALPHA, uvs=uv, what=evplp.SURFACE_PHOTONS)
        c.synchronize()
    got = st.cpu().numpy().view(evplp.SURFACE_STATE_DTYPE).reshape(-1)
    covered = hits["triangle"] >= 0
    assert 0.2 < covered.mean() < 0.9
    assert got.tobytes() == want.tobytes(), np.nonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])[0][:8]
    assert got[~covered].tobytes() == bytes(48 * int((~covered).sum())), "an uncovered sample's state stays fresh"
    assert (got["pm_calls"][covered] == 1).all() and (got["flags"] == 0).all() and (got["n"][covered] >= F(ALPHA) * F(k)).mean() > 0.1
    assert (got["radius2"][covered] > 0).all() and (got["radius2"][covered] <= f.r0sq).all() and len(np.unique(bits(got["radius2"][covered]))) > 100
    assert st_rows.cpu().numpy().tobytes() == got.tobytes(), "EVPLP_LIGHTMAP_BAND of one row"
    cov = covered.reshape(H, W, S * S).sum(-1)
    assert np.array_equal(tex["coverage"][cov > 0], (cov[cov > 0] / F(S * S)).astype(F)) and np.isfinite(tex.view(F)).all() and tex["pm"].max() > 1e-5
    nxt = after.cpu().numpy().view(evplp.SURFACE_STATE_DTYPE).reshape(-1)
    assert (nxt["flags"] == 0).all() and (nxt["pm_calls"][covered] == 2).all() and (nxt["radius2"][covered] <= got["radius2"][covered]).all() and nxt["n"].sum() > got["n"].sum()
    say(f"lightmap {W} x {H} at S = {S}: {int(covered.sum())} covered samples, {int((got['n'][covered] >= F(ALPHA) * F(k)).sum())} with k photons or more, mean radius2 / r0sq {float(got['radius2'][covered].mean() / f.r0sq):.3f}")
