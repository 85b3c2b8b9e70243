"""The progressive surface gather on the device (evplp_gather_surface_progressive, evplp_surface_resolve, the progressive bake): per-point
photon statistics with per-point radii, on test_gpu_surface.py's sizes -- scenes.box_room, the oracle's 64 x 48 G-buffer as 3 072 points,
2 000 x 4 record slots of which the VPL half reads the first 160 x 4; the records are the oracle's light paths of four seeds.

  1  alpha = 1, three iterations, modes 0 / 4 / 5: radius2 keeps r0sq's bits, n is the sum of the plain calls' photons, vpl and lit_sum
     are the fp32 running sums of the plain calls' bytes, the resolved pm is the mean of the plain pm under the project's bars.
  2  alpha = 2/3, four iterations against a numpy brute force over ALL photons: the float32 inside test at the point's own radius2, M per
     point per iteration exact, n and radius2 bit for bit through the float32 restatement of the rule, tau against the float64 fragment of
     tests/shading_domain.py under the photon half's own bar (K_GPU_SPLAT).  The bar of a sum: the fragments' bars, M 2^-24 of their
     absolute sum for the additions in visiting order, and per iteration 2 * 2^-24 |tau| for (tau + Phi) ratio's two roundings -- the
     construction test_gpu_surface.py uses for its whole set; an undecided fragment (one a cut's margin from a branch) takes its point out
     of the tau comparison for good, and out of nothing else.
  3  hostile states in one wave and one lane of the next; 4 a point's 48 bytes; 5 refusals; 6 the lightmap.

Measured on an MI355X, 2026-10-21 (`pytest -s -m gpu tests/test_gpu_surface_progressive.py` prints them).  alpha = 1: 20 038 photons kept,
resolved pm against the mean of the plain calls 6.31e-8 / 6.36e-8 / 6.30e-8 relative L2 in modes 0 / 4 / 5 against the 1e-5 bar.  alpha =
2/3: M per iteration 6 564, 4 761, 3 991, 3 435; tau error / bar at its worst 0.164 / 0.224 / 0.285 (K = 18), no undecided fragment; mean
radius2 / r0sq after four iterations 0.497.  Hostile states: M 1 .. 10, 21 flagged, 7 stencilled, tau error / bar 0.409.  Lightmap 32 x 32
at S = 2: 4.64e-8 (VPL) and 6.00e-8 (photons) relative L2 from the mean of three bakes.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import shading_domain as sd
from test_gpu_lightmap import band, bits, lr, packed_uvs
from test_gpu_parity import REL_L2, assert_image_close, rel_l2
from test_gpu_shading_domain import K_GPU_SPLAT
from test_gpu_surface import NPATHS, P, Room, dot32, floor_box, floor_points, hostile_records, room_context

pytestmark = pytest.mark.gpu

F = np.float32
MODES = (0, 4, 5)
SEEDS = (5, 6, 7, 8)
ALPHA = 2.0 / 3.0


def say(*a):
    print("[surface progressive]", *a, flush=True)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def restate(state, M, alpha, r0sq, live):
    """include/evplp.h's rule over arrays, every operation a float32 one; tau is left alone (the caller holds it in float64).  Returns the
    new state and the float32 ratio per point (1 where M = 0)."""
    s = state.copy()
    alpha, r0sq = F(alpha), F(r0sq)
    first = live & (s["pm_calls"] == 0)
    s["radius2"][first] = r0sq
    hit = live & (M > 0)
    m = M.astype(F)
    with np.errstate(all="ignore"):
        nn = s["n"] + alpha * m
        ratio = np.where(hit, nn / (s["n"] + m), F(1)).astype(F)
    s["radius2"] = np.where(hit, s["radius2"] * ratio, s["radius2"])
    s["n"] = np.where(hit, nn, s["n"])
    s["pm_calls"] += live.astype(np.uint32)
    return s, ratio


def usable_photons(rec, slots):
    ok = (rec["flags"][:slots] & 2) != 0
    ok[0] = False
    return np.nonzero(ok)[0]


def inside_own(rec, slots, X, radius2):
    """[usable photons, points] of the float32 test at each point's own radius2, and the photons' slots"""
    k = usable_photons(rec, slots)
    dv = rec["pos"][k][:, None, :].astype(F) - X[None, :, :].astype(F)
    return ~(dot32(dv, dv) > radius2[None, :].astype(F)), k


def phi_f64(mode, fpd, pts, rec, inside, slots_of):
    """per point: the float64 sum of the fragment without InvPi / r^2 over the photons inside, its bar, and whether every fragment is decided"""
    flat = np.ascontiguousarray(pts).view(F).reshape(-1, 16)
    pix = sd.pixels_of([flat[:, 4 * k:4 * k + 4] for k in range(4)])
    wide = dict(fpd, photon_radius=4.0 * float(fpd["photon_radius"]))           # (the float64 radius test of the fragment lets every pair in)
    r = float(F(wide["photon_radius"]))
    unk = (r * r) / sd.INV_PI
    n = len(pts)
    phi = np.zeros((n, 3)); bar = np.zeros((n, 3)); mag = np.zeros((n, 3)); decided = np.ones(n, bool)
    for row in np.nonzero(inside.any(1))[0]:
        idx = np.nonzero(inside[row])[0]
        sub = SimpleNamespace(pos=pix.pos[idx], stencil=pix.stencil[idx], nrm=pix.nrm[idx], rd=pix.rd[idx], rs=pix.rs[idx], e=pix.e[idx])
        k = int(slots_of[row])
        val, kappa, lam, dec, ins, _ = sd.photon_frag_f64(mode, wide, sub, rec[k], rec[k - 1])
        assert ins.all()
        val = val * unk
        phi[idx] += val; bar[idx] += sd.bar(val, kappa, lam, K_GPU_SPLAT, True); mag[idx] += np.abs(val); decided[idx] &= dec
    return phi, bar + inside.sum(0)[:, None] * 2.0 ** -24 * mag, decided


# ---------------------------------------------------------------------------------------------------------------- the room, once
@pytest.fixture(scope="module")
def prog(evplp, oracle):
    room = Room(evplp)
    room.recs = [room.osc.trace_light_paths(s, NPATHS, P) for s in SEEDS]
    room.pts["valid"][5::97] = 0.0                  # (the room is closed: every pixel shows a surface) stencilled points among them
    room.valid = room.pts["valid"] != 0
    assert room.valid.sum() > 0.9 * room.n and not room.valid.all()
    room.r0sq = F(room.radius) * F(room.radius)
    room.plain = {}
    with room_context(evplp, room) as c:
        for mode in MODES:
            fp = evplp.frame_params(**room.params(mode))
            room.plain[mode] = []
            for rec in room.recs[:3]:
                c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
                room.plain[mode].append(c.gather_surface(room.pts, fp))
    return room


def iterate(evplp, c, room, mode, alpha, count, states=None, pts=None):
    """the states after each of `count` iterations over room.recs"""
    pts = room.pts if pts is None else pts
    st = np.zeros(len(pts), evplp.SURFACE_STATE_DTYPE) if states is None else states
    fp = evplp.frame_params(**room.params(mode))
    out = []
    for rec in room.recs[:count]:
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        st = c.gather_surface_progressive(pts, fp, st, alpha=alpha)
        out.append(st)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("mode", MODES)
def test_alpha_one_accumulates_the_plain_calls(evplp, prog, mode):
    with room_context(evplp, prog) as c:
        st = iterate(evplp, c, prog, mode, 1.0, 3)[-1]
        res = c.surface_resolve(st)
    plain = prog.plain[mode]
    v = prog.valid
    assert st[~v].tobytes() == bytes(48 * int((~v).sum())), "a stencilled point's state stays fresh"
    assert (st["flags"] == 0).all() and (st["vpl_calls"][v] == 3).all() and (st["pm_calls"][v] == 3).all()
    assert (bits(st["radius2"][v]) == bits(np.asarray([prog.r0sq]))[0]).all(), "ratio is exactly 1: radius2 keeps r0sq's bits"
    total = sum(p["photons"].astype(np.float64) for p in plain)
    assert np.array_equal(st["n"].astype(np.float64), total) and total.sum() > 15000
    acc = np.zeros((prog.n, 3), F); lit = np.zeros(prog.n, F)
    for p in plain:
        acc = acc + p["vpl"]; lit = lit + p["lit"]
    assert np.array_equal(bits(st["vpl"]), bits(acc)) and np.array_equal(bits(st["lit_sum"]), bits(lit)), "the fp32 running sums of the plain calls' bytes"
    assert np.array_equal(bits(res["vpl"]), bits(acc / F(3))) and np.array_equal(bits(res["lit"]), bits(lit / F(3))) and np.array_equal(res["photons"], st["n"])
    mean = sum(p["pm"].astype(np.float64) for p in plain) / 3.0
    say(f"alpha = 1, mode {mode}: resolved pm against the mean of three plain calls, rel L2 {rel_l2(res['pm'], mean):.2e} (bar {REL_L2}); {int(total.sum())} photons kept")
    assert np.abs(mean).max() > 1e-4
    assert_image_close(res["pm"], mean, what=f"resolved pm, mode {mode}")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.fixture(scope="module")
def walk(evplp, prog):
    """the brute force of four iterations at alpha = 2/3: per iteration the inside matrix at the restated radii, M, and the restated state"""
    st = np.zeros(prog.n, evplp.SURFACE_STATE_DTYPE)
    steps = []
    for rec in prog.recs:
        r2 = np.where(st["pm_calls"] == 0, prog.r0sq, st["radius2"]).astype(F)
        inside, slots = inside_own(rec, NPATHS * P, prog.pts["pos"], r2)
        inside &= prog.valid[None, :]
        M = inside.sum(0)
        new, ratio = restate(st, M, ALPHA, prog.r0sq, prog.valid)
        steps.append(SimpleNamespace(rec=rec, inside=inside, slots=slots, M=M, before=st, after=new, ratio=ratio))
        st = new
    return steps


@pytest.mark.parametrize("mode", MODES)
def test_four_iterations_against_the_brute_force(evplp, prog, walk, mode):
    with room_context(evplp, prog) as c:
        got = iterate(evplp, c, prog, mode, ALPHA, 4)
    v = prog.valid
    tau = np.zeros((prog.n, 3)); tbar = np.zeros((prog.n, 3)); decided = np.ones(prog.n, bool)
    worst = 0.0
    for it, (g, w) in enumerate(zip(got, walk)):
        # M: n grows by fl(alpha M), which tells M apart while n is small; and n, radius2 bit for bit say it again
        grown = (g["n"].astype(np.float64) - w.before["n"].astype(np.float64)) / float(F(ALPHA))
        assert np.array_equal(np.rint(grown).astype(np.int64), w.M), (it, np.nonzero(np.rint(grown) != w.M)[0][:8])
        assert np.array_equal(bits(g["n"]), bits(w.after["n"])) and np.array_equal(bits(g["radius2"]), bits(w.after["radius2"])), it
        assert np.array_equal(g["pm_calls"], w.after["pm_calls"]) and (g["flags"] == 0).all() and (g["vpl_calls"][v] == it + 1).all()
        start = np.where(w.before["pm_calls"] == 0, prog.r0sq, w.before["radius2"])
        assert (g["radius2"][v] <= start[v]).all() and (g["radius2"][v & (w.M > 0)] < start[v & (w.M > 0)]).all(), "a radius never grows, and shrinks where photons arrive"
        assert np.array_equal(bits(g["radius2"][v & (w.M == 0)]), bits(start[v & (w.M == 0)].astype(F)))
        phi, pbar, dec = phi_f64(mode, prog.params(mode), prog.pts, w.rec, w.inside, w.slots)
        ratio = w.ratio.astype(np.float64)[:, None]
        hit = (w.M > 0)[:, None]
        tau = np.where(hit, (tau + phi) * ratio, tau)
        tbar = np.where(hit, (tbar + pbar) * ratio + 2.0 * 2.0 ** -24 * np.abs(tau), tbar)
        decided &= dec
        err = np.abs(g["tau"].astype(np.float64) - tau)
        ok = decided & v
        r = float((err[ok] / (tbar[ok] + 1e-20)).max())
        worst = max(worst, r)
        assert np.isfinite(g["tau"]).all() and r <= 1.0, (mode, it, r)
        assert (g["tau"][~v] == 0).all()
    assert decided[v].mean() > 0.9 and walk[0].M.sum() > 5000 and walk[3].M.sum() < walk[0].M.sum()
    say(f"alpha = 2/3, mode {mode}: M per iteration {[int(w.M.sum()) for w in walk]}, tau error / bar at its worst {worst:.3f} (K = {K_GPU_SPLAT}), "
        f"{int((~decided & v).sum())} points with an undecided fragment; mean radius2 / r0sq after four: {float(got[-1]['radius2'][v].mean() / prog.r0sq):.3f}")


# ---------------------------------------------------------------------------------------------------------------- 3
def test_hostile_states_in_one_wave(evplp, oracle):
    """65 points on the line y = 0 of the floor, so that a photon at (x, +-d, 0) has dv = (0, +-d, 0) exactly: d^2 == radius2 is inside,
    the next d up whose square rounds above radius2 is outside"""
    scene = sd.floor_scene()
    lo, hi = floor_box(scene)
    n = 65
    r0 = 0.25
    r0sq = F(r0) * F(r0)
    up = F(np.inf)
    X = np.zeros((n, 3), F); X[:, 0] = (-10.0 + 0.28 * np.arange(n)).astype(F)
    assert X[:, 0].max() < hi[0] and X[:, 0].min() > lo[0]
    kinds = ["r0sq", "fresh", "above", "tiny", "denormal", "zero", "nan", "seeded", "stencil"]
    kind = [kinds[i % len(kinds)] for i in range(n)]
    kind[20] = "nan_point"; kind[33] = "inf_eye"; kind[64] = "tiny"
    seed = {"r0sq": r0sq, "above": np.nextafter(r0sq, up), "tiny": F(2.0 ** -40), "denormal": F(2.0 ** -140), "zero": F(0), "nan": F(np.nan), "seeded": F(0.1875) * F(0.1875)}
    st = np.zeros(n, evplp.SURFACE_STATE_DTYPE)
    pts = floor_points(evplp, X)
    eyes = np.ascontiguousarray(np.broadcast_to(np.asarray(sd.CAMERA, F), (n, 3))).copy()
    photons = []
    for i, k in enumerate(kind):
        if k in seed:
            st[i] = ((0.5, 0.25, 0.125), seed[k], (1.0, 2.0, 3.0), 6.0, 4.0, 2, 1, 0)
        elif k != "fresh":
            st[i] = ((0.5, 0.25, 0.125), r0sq * F(0.5), (1.0, 2.0, 3.0), 6.0, 4.0, 2, 1, 0)
        if k == "stencil":
            pts["valid"][i] = 0.0
            st[i:i + 1].view(np.uint8)[:] = 0xA5
        if k == "nan_point":
            pts["pos"][i, 2] = np.nan
        if k == "inf_eye":
            eyes[i, 0] = np.inf
        r2 = r0sq if k == "fresh" else st["radius2"][i]
        if k in ("zero", "nan", "stencil", "nan_point", "inf_eye", "above"):
            r2 = r0sq
        d = F(np.sqrt(np.float64(r2)))
        assert F(d * d) == r2, (k, d, r2)                       # the seeded squares are exact
        out = np.nextafter(d, up)
        if not F(out * out) > r2:
            out = F(d * F(1.0 + 2.0 ** -8))                     # (a denormal square moves only with its ninth bit)
        assert F(out * out) > r2 and F(X[i, 1] + d) == d
        photons.append([X[i, 0], d, 0.0]); photons.append([X[i, 0], -out, 0.0])
    # ... and 300 more along the line, for counts that differ from point to point
    rng = np.random.RandomState(12)
    more = np.zeros((300, 3), F); more[:, 0] = rng.uniform(-10.2, 8.2, 300).astype(F); more[:, 1] = rng.uniform(-0.3, 0.3, 300).astype(F)
    photons = np.concatenate([np.asarray(photons, F), more])
    rec = hostile_records(photons)
    slots = 2 * len(photons)
    flagged = np.asarray([k in ("above", "zero", "nan", "nan_point", "inf_eye") for k in kind])
    stencil = np.asarray([k == "stencil" for k in kind])
    live = ~flagged & ~stencil
    r2 = np.where(st["pm_calls"] == 0, r0sq, st["radius2"]).astype(F)
    inside, slot_of = inside_own(rec, slots, X, np.where(live, r2, F(0)))
    inside &= live[None, :]
    M = inside.sum(0)
    # the photon on the radius is inside, the one an ulp beyond is outside: rows 2 i and 2 i + 1 are point i's own
    own = np.arange(n)
    assert inside[2 * own, own][live].all() and not inside[2 * own + 1, own].any()
    want, ratio = restate(st, M, ALPHA, r0sq, live)
    mode = 5
    kw = dict(camera_pos=sd.CAMERA, mis_mode=mode, pdf_mc=0.02, clamping_value=0.02, photon_radius=r0, num_light_paths=len(photons), num_vpl_light_paths=1, photons_per_path=2)
    with evplp.Context(sd.W, sd.H, len(photons), 1, 2, deterministic=True) as c:
        scene.upload(c)
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
        got = c.gather_surface_progressive(pts, evplp.frame_params(**kw), st, alpha=ALPHA, eyes=eyes)
        res = c.surface_resolve(got)
    assert got[stencil].tobytes() == st[stencil].tobytes(), "a stencilled state keeps all 48 bytes"
    keep = st[flagged].copy(); keep["flags"] |= 1
    assert got[flagged].tobytes() == keep.tobytes(), "a flagged state keeps every other byte"
    assert np.array_equal(bits(got["n"][live]), bits(want["n"][live])) and np.array_equal(bits(got["radius2"][live]), bits(want["radius2"][live])), np.nonzero(bits(got["n"]) != bits(want["n"]))[0]
    assert np.array_equal(got["pm_calls"][live], want["pm_calls"][live]) and (got["vpl_calls"][live] == st["vpl_calls"][live] + 1).all() and (got["flags"][live] == 0).all()
    assert np.array_equal(bits(got["vpl"][live]), bits(st["vpl"][live])) and np.array_equal(bits(got["lit_sum"][live]), bits(st["lit_sum"][live])), "no usable VPL: the sums stay"
    assert (M[live] >= 1).all() and got["radius2"][np.asarray(kind) == "denormal"].max() < 2.0 ** -126
    phi, pbar, dec = phi_f64(mode, kw, pts, rec, inside, slot_of)
    r64 = ratio.astype(np.float64)[:, None]
    tau = (st["tau"].astype(np.float64) + phi) * r64
    tbar = pbar * r64 + 3.0 * 2.0 ** -24 * np.abs(tau) + 1e-20
    ok = live & dec
    worst = float((np.abs(got["tau"].astype(np.float64) - tau)[ok] / tbar[ok]).max())
    say(f"hostile states: M {M[live].min()} .. {M[live].max()}, {int(flagged.sum())} flagged, {int(stencil.sum())} stencilled, tau error / bar at its worst {worst:.3f}")
    assert ok.sum() > 30 and worst <= 1.0
    flat = res.view(F).reshape(-1, 8)
    assert all(flat[i].tolist() == [0, 0, 0, -1, 0, 0, 0, -1] for i in np.nonzero(flagged)[0])


# ---------------------------------------------------------------------------------------------------------------- 4
def test_a_points_48_bytes_do_not_depend_on_the_batch_the_form_or_the_buckets(evplp, prog, monkeypatch):
    import torch
    mode = 5
    fp = evplp.frame_params(**prog.params(mode))

    def second(c, pts, states):
        c.upload(evplp.BUF_RECORDS, prog.recs[1].astype(evplp.RECORD_DTYPE))
        return c.gather_surface_progressive(pts, fp, states, alpha=ALPHA)
    n = evplp.SURFACE_CHUNK + 65
    src = (np.arange(n) * 7 + 3) % prog.n
    with room_context(evplp, prog) as c:
        first = iterate(evplp, c, prog, mode, ALPHA, 1)[0]              # radii that differ from point to point
        base = second(c, prog.pts, first)
        assert len(np.unique(bits(base["radius2"][prog.valid]))) > 20      # (a radius2 is a function of the point's counts (M1, M2): dozens of values, not thousands)
        assert second(c, prog.pts, first).tobytes() == base.tobytes(), "two runs"
        for i in (0, 777, prog.n - 1):
            assert second(c, prog.pts[i:i + 1], first[i:i + 1]).tobytes() == base[i:i + 1].tobytes(), i
        big = second(c, prog.pts[src], first[src])
        assert big.tobytes() == base[src].tobytes(), np.nonzero([g.tobytes() != x.tobytes() for g, x in zip(big, base[src])])[0][:8]
        # the device form, across the chunk boundary too
        d = torch.from_numpy(np.ascontiguousarray(prog.pts[src]).view(F).reshape(-1, 16)).cuda()
        s = torch.from_numpy(np.ascontiguousarray(first[src]).view(F).reshape(-1, 12).copy()).cuda()
        torch.cuda.synchronize()
        out = second(c, d, s)
        r = c.surface_resolve(out)
        c.synchronize()
        assert out.data_ptr() == s.data_ptr() and out.cpu().numpy().tobytes() == base[src].tobytes(), "the device form"
        assert r.cpu().numpy().tobytes() == c.surface_resolve(base[src]).tobytes()
    monkeypatch.setenv("EVPLP_SURFACE_GRID_BITS", "1")                  # two buckets
    with room_context(evplp, prog) as c:
        assert second(c, prog.pts, first).tobytes() == base.tobytes(), "EVPLP_SURFACE_GRID_BITS = 1"


# ---------------------------------------------------------------------------------------------------------------- 5
def test_refusals_leave_the_states_and_the_context_untouched(evplp, prog):
    import torch
    L = evplp.lib()
    INV = evplp.ERR_INVALID
    BOTH = evplp.SURFACE_VPL | evplp.SURFACE_PHOTONS
    pts = prog.pts[:8].copy()
    st = np.full(8 * 48, 0x5A, np.uint8)
    xp, sp = pts.ctypes.data, st.ctypes.data

    def prm(**kw):
        p = prog.params(5); p.update(kw)
        return C.byref(evplp.frame_params(**p))
    a = C.c_float(ALPHA)
    with room_context(evplp, prog) as c:
        base = c.gather_surface_progressive(pts, evplp.frame_params(**prog.params(5)), np.zeros(8, evplp.SURFACE_STATE_DTYPE), alpha=ALPHA)
        d = torch.from_numpy(pts.view(F).reshape(-1, 16)).cuda()
        o = torch.full((8 * 12 + 4,), 7.0, dtype=torch.float32, device="cuda")
        for form, px, ps in ((L.evplp_gather_surface_progressive, xp, sp), (L.evplp_gather_surface_progressive_device, C.c_void_p(d.data_ptr()), C.c_void_p(o.data_ptr()))):
            for mode in (1, 2, 3):
                assert form(c._h, prm(mis_mode=mode), BOTH, a, px, None, 8, ps) == INV and b"pdf_mc" in L.evplp_last_error(c._h), mode
            assert form(c._h, prm(mis_mode=6), BOTH, a, px, None, 8, ps) == INV
            for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
                assert form(c._h, prm(), BOTH, C.c_float(bad), px, None, 8, ps) == INV and b"alpha" in L.evplp_last_error(c._h), bad
            assert form(c._h, prm(), BOTH, a, px, None, 8, None) == INV and form(c._h, prm(), BOTH, a, None, None, 8, ps) == INV
            assert form(c._h, None, BOTH, a, px, None, 8, ps) == INV and form(c._h, prm(), 0, a, px, None, 8, ps) == INV and form(c._h, prm(), 4, a, px, None, 8, ps) == INV
            assert form(c._h, prm(), BOTH, a, px, None, -1, ps) == INV
            assert form(c._h, prm(photon_radius=0.0), BOTH, a, px, None, 8, ps) == INV and form(c._h, prm(num_light_paths=NPATHS + 1), BOTH, a, px, None, 8, ps) == INV
            assert form(c._h, prm(), BOTH, a, px, None, 0, ps) == evplp.OK and form(c._h, prm(), BOTH, a, None, None, 0, None) == evplp.OK
        assert L.evplp_gather_surface_progressive_device(c._h, prm(), BOTH, a, C.c_void_p(d.data_ptr()), None, 8, C.c_void_p(o.data_ptr() + 4)) == INV
        assert b"states are not 16-byte aligned" in L.evplp_last_error(c._h)
        assert L.evplp_gather_surface_progressive(c._h, prm(), BOTH, a, xp, None, 8, None) == INV and b"null states" in L.evplp_last_error(c._h)
        assert L.evplp_surface_resolve_device(c._h, C.c_void_p(o.data_ptr() + 4), 8, C.c_void_p(o.data_ptr())) == INV and L.evplp_surface_resolve(c._h, None, 8, sp) == INV
        c.synchronize()
        assert (st == 0x5A).all() and (o.cpu().numpy() == 7.0).all(), "a refused call writes nothing"
        again = c.gather_surface_progressive(pts, evplp.frame_params(**prog.params(5)), np.zeros(8, evplp.SURFACE_STATE_DTYPE), alpha=ALPHA)
        assert again.tobytes() == base.tobytes(), "the context is usable afterwards"


# ---------------------------------------------------------------------------------------------------------------- 6
def test_lightmap_three_iterations_then_resolve(evplp, prog):
    import torch
    W = H = 32
    S = 2
    mode = 0
    uv = packed_uvs(prog.scene)
    fp = evplp.frame_params(**prog.params(mode))
    n = W * H * S * S

    def run(c):
        st = torch.zeros((n, 12), dtype=torch.float32, device="cuda")
        for rec in prog.recs[:3]:
            c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
            c.bake_lightmap_progressive_device(fp, st, W, H, S, alpha=1.0, uvs=uv)
        c.synchronize()
        return st
    with room_context(evplp, prog) as c:
        plain = []
        for rec in prog.recs[:3]:
            c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
            plain.append(c.bake_lightmap(fp, W, H, S, uvs=uv))
        st = run(c)
        got = {g: c.bake_lightmap_resolve(st, W, H, S, gutter=g) for g in (0, 2)}
        dev = c.bake_lightmap_resolve_device(st, W, H, S, gutter=2)
        c.synchronize()
        with band(W * S * S):                                           # one texel row per band
            st_rows = run(c)
            rows = c.bake_lightmap_resolve(st_rows, W, H, S, gutter=2)
    base = got[0]
    cov = plain[0]["coverage"]
    assert 0.2 < (cov > 0).mean() < 0.9 and ((cov > 0) & (cov < 1)).sum() > 20, "covered, empty and partly covered texels"
    assert np.array_equal(bits(base["coverage"]), bits(cov)), "coverage is exact"
    assert (bits(base.view(F).reshape(H, W, 8)[cov == 0]) == 0).all(), "an uncovered texel is 32 zero bytes"
    states = st.cpu().numpy().view(evplp.SURFACE_STATE_DTYPE).reshape(H, W, S * S)
    hits = lr.rasterise(uv, 0, W, H, S, evplp.HIT_DTYPE).reshape(H, W, S * S)
    fresh = states.view(np.uint8).reshape(H, W, S * S, 48).any(-1)
    assert np.array_equal(fresh, hits["triangle"] >= 0), "an uncovered sample's state stays fresh"
    mean_vpl = sum(p["vpl"].astype(np.float64) for p in plain) / 3.0
    mean_pm = sum(p["pm"].astype(np.float64) for p in plain) / 3.0
    total = sum(p["photons"].astype(np.float64) for p in plain)
    say(f"lightmap {W} x {H} at S = {S}: VPL rel L2 {rel_l2(base['vpl'], mean_vpl):.2e}, photons rel L2 {rel_l2(base['pm'], mean_pm):.2e} (bar {REL_L2}); {int(total.sum())} photons per texel summed")
    assert np.abs(mean_vpl).max() > 1e-3 and np.abs(mean_pm).max() > 1e-5 and total.sum() > 100
    assert_image_close(base["vpl"], mean_vpl, what="resolved texels, vpl")
    assert_image_close(base["pm"], mean_pm, what="resolved texels, pm")
    assert np.allclose(base["photons"].astype(np.float64), total, rtol=2.0 ** -21, atol=0.0), "photons: the texel's mean of n, the sum over the iterations"
    assert got[2].tobytes() == lr.gutter(base, 2).tobytes(), "gutter 2: the bake's rule, byte for byte"
    assert dev.cpu().numpy().tobytes() == got[2].tobytes(), "the device form of the resolve"
    assert st_rows.cpu().numpy().tobytes() == st.cpu().numpy().tobytes() and rows.tobytes() == got[2].tobytes(), "EVPLP_LIGHTMAP_BAND of one row"
