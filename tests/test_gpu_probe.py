"""The probe gather on the device (evplp_gather_probes, its device form) against the oracle's visibility and the float64 restatement of
tests/probe_restate.py.

Scene scenes.box_room, records traced by the oracle: 160 paths x 4 = 640 slots, two full slices of EVPLP_PROBE_SLICE_SLOTS and a half;
197 free points, three waves and a ragged one.  The references are computed once (class Reference):
  visibility  the shadow ray of every pair that passes the kernel's own float32 cosine test (origin pos_k, direction -(pos_k - x), tmin
              0.0001f, tmax 1.0f - 0.0001f) through evo_occluded_brute and evo_occluded.  A pair on which the two disagree is set aside;
              at most 0.5 % may be, and with these seeds none is.  `lit` must equal the count exactly, and evplp_trace_occluded's count.
  values      each of the 27 numbers within the sum over its lit pairs of bar(term, kappa, lam, 2 K_ORACLE_PROBE, hw_pow=True) plus
              lit 2^-24 sum |term| for the float32 accumulation (which also covers the one division); an undecided pair widens the bar
              by its own magnitude, and at most 8 per probe may be undecided (shading_domain.check_caps)."""
import ctypes as C

import numpy as np
import pytest

import oracle_api as oa
import probe_restate as pr
import scenes
import shading_domain as sd
from probe_domain import MIN_DISTANCE, Reference, check_values, say      # (Reference holds the kernel to K_GPU_PROBE = 2 K_ORACLE_PROBE)

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 64, 48                        # the contexts' frame: only the last test renders
NPATHS, P = 160, 4
SLOTS = NPATHS * P
N_PROBES = 197


def free_points(rng, n):
    """points inside the room [0, 10] x [0, 8] x [0, 5] (some lie inside a box: a probe may be anywhere)"""
    return (rng.uniform(0.05, 0.95, size=(n, 3)) * np.array([10.0, 8.0, 5.0])).astype(F)


@pytest.fixture(scope="module")
def room():
    return scenes.box_room(seed=3, n_boxes=6, tess=2, aspect=W / H)


@pytest.fixture(scope="module")
def records(oracle, room):
    rec = oa.Scene(room).trace_light_paths(5, NPATHS, P)
    usable = (rec["flags"] & 1) != 0
    assert usable[:512].sum() > 100 and usable[512:].sum() > 30 and (~usable).sum() > 30, "usable and unusable slots in every slice"
    assert (rec["rho_s"][usable] != 0).any(), "some VPLs carry a Phong lobe"
    return rec


@pytest.fixture(scope="module")
def probes():
    return free_points(np.random.RandomState(17), N_PROBES)


@pytest.fixture(scope="module")
def ref(oracle, room, records, probes):
    r = Reference(oa.Scene(room), records, probes, per_path=P)
    assert r.aside_rays.sum() <= 0.005 * len(r.rays)
    assert r.aside_rays.sum() == 0, "with these seeds evo_occluded and evo_occluded_brute agree on every shadow ray"
    _, _, lit, und = r.expect(NPATHS)
    sd.check_caps([int(u) for u in und], int(lit.sum()))
    say(f"reference: {len(r.slots)} usable of {SLOTS} slots, {len(r.rays)} shadow rays, {int(r.lit.sum())} lit pairs, {int(und.sum())} undecided")
    assert 0.2 < r.lit.sum() / len(r.rays) < 0.95, "occluded and lit pairs both"
    return r


def context(evplp, sd_, rec=None, paths=NPATHS):
    c = evplp.Context(W, H, paths, paths, P, deterministic=True)
    sd_.upload(c)
    if rec is not None:
        c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))
    return c


@pytest.fixture(scope="module")
def base(evplp, room, records, probes):
    """the batch of 197 on the records as traced: what every other form is compared with, byte for byte"""
    with context(evplp, room, records) as c:
        return c.gather_probes(probes, NPATHS, P, MIN_DISTANCE)


# ---- 1: visibility and values
def test_lit_counts_equal_the_occlusion_query_and_the_brute_force(evplp, room, records, probes, ref, base):
    with context(evplp, room, records) as c:
        occ = c.trace_occluded(ref.rays)
    assert occ.max() <= 1
    keep = ~ref.aside_rays
    assert np.array_equal(occ[keep], ref.occluded_rays[keep]), "evplp_trace_occluded answers these rays as evo_occluded_brute does"
    per_probe = np.zeros(N_PROBES, np.int64)
    np.add.at(per_probe, ref.where[occ == 0, 1], 1)
    assert np.array_equal(base["lit"], per_probe.astype(F)), np.nonzero(base["lit"] != per_probe)[0][:8]
    assert np.array_equal(base["lit"], ref.expect(NPATHS)[2].astype(F))


def test_values_stay_within_the_bar_of_the_restatement(ref, base):
    lit = check_values(base, ref, NPATHS, "197 probes, 640 slots")
    assert (lit > 20).sum() > 150 and np.abs(base["c"]).max() > 1e-3 and np.isfinite(base["c"]).all()


# ---- 2: a probe's bytes
def test_a_probes_bytes_do_not_depend_on_the_batch(evplp, room, records, probes, base):
    with context(evplp, room, records) as c:
        for i in (0, 5, 196):
            assert c.gather_probes(probes[i:i + 1], NPATHS, P, MIN_DISTANCE).tobytes() == base[i:i + 1].tobytes(), i
        for n in (63, 64, 65):
            assert c.gather_probes(probes[:n], NPATHS, P, MIN_DISTANCE).tobytes() == base[:n].tobytes(), n
        # across the chunk boundary: copies of the 197 in another order, probe 5 at index EVPLP_PROBE_CHUNK + 5
        n = evplp.PROBE_CHUNK + 70
        src = (np.arange(n) * 7 + 3) % N_PROBES
        src[evplp.PROBE_CHUNK + 5] = 5
        got = c.gather_probes(probes[src], NPATHS, P, MIN_DISTANCE)
        assert got[evplp.PROBE_CHUNK + 5].tobytes() == base[5].tobytes()
        assert got.tobytes() == base[src].tobytes(), np.nonzero([g.tobytes() != b.tobytes() for g, b in zip(got, base[src])])[0][:8]


def test_the_device_form_gives_the_host_forms_bytes_without_a_wait_between_calls(evplp, room, records, probes, base):
    import torch
    with context(evplp, room, records) as c:
        d = torch.from_numpy(probes).cuda()
        torch.cuda.synchronize()
        a = c.gather_probes(d, NPATHS, P, MIN_DISTANCE)
        b = c.gather_probes(d[:65], NPATHS, P, MIN_DISTANCE)          # enqueued behind the first without a wait in between
        c.synchronize()
        assert isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and tuple(a.shape) == (N_PROBES, 28)
        assert a.cpu().numpy().tobytes() == base.tobytes() and b.cpu().numpy().tobytes() == base[:65].tobytes()


# ---- 3: slices
def test_slot_counts_below_one_slice_and_at_an_exact_multiple(evplp, room, records, probes, ref, base):
    with context(evplp, room, records) as c:
        for paths in (32, 128):                               # 128 slots: half a slice; 512: exactly two
            got = c.gather_probes(probes, paths, P, MIN_DISTANCE)
            lit = check_values(got, ref, paths, f"{paths * P} slots")
            assert lit.sum() > 0 and got.tobytes() != base.tobytes()
        assert c.gather_probes(probes, NPATHS, P, MIN_DISTANCE).tobytes() == base.tobytes(), "the larger scratch of an earlier call changes nothing"


def test_unusable_slots_and_a_last_partial_slice_alone(evplp, room, records, probes, ref, base):
    dark = records.copy(); dark["flags"] = 0; dark["flux"] = sd.BIG          # (ruinous if it were read)
    tail = records.copy(); tail["flags"][:512] = 0; tail["flux"][:512] = sd.BIG
    keep = np.arange(SLOTS) >= 512
    with context(evplp, room, dark) as c:
        got = c.gather_probes(probes, NPATHS, P, MIN_DISTANCE)
        assert (got["c"] == 0).all() and (got["lit"] == 0).all()
        c.upload(evplp.BUF_RECORDS, tail.astype(evplp.RECORD_DTYPE))
        got = c.gather_probes(probes, NPATHS, P, MIN_DISTANCE)
        lit = check_values(got, ref, NPATHS, "usable records in the last, partial slice only", keep)
        assert lit.sum() > 500


# ---- 4: invalid probes, refusals
def test_probes_that_are_not_finite_are_not_walked_and_leave_their_neighbours_alone(evplp, room, records, probes, base):
    x = probes.copy()
    bad = {3: (0, np.nan), 64: (1, np.inf), 130: (2, -np.inf), 196: (0, np.nan)}
    for i, (axis, v) in bad.items():
        x[i, axis] = v
    with context(evplp, room, records) as c:
        got = c.gather_probes(x, NPATHS, P, MIN_DISTANCE)
        import torch
        dev = c.gather_probes(torch.from_numpy(x).cuda(), NPATHS, P, MIN_DISTANCE)
        c.synchronize()
        assert dev.cpu().numpy().tobytes() == got.tobytes()
    ok = np.ones(N_PROBES, bool); ok[list(bad)] = False
    assert (got["lit"][~ok] == -1).all() and (got["c"][~ok] == 0).all()
    assert got[ok].tobytes() == base[ok].tobytes()


def test_refusals_leave_the_context_usable_and_write_nothing(evplp, room, records, probes, base):
    L = evplp.lib()
    x = probes[:8].copy()
    out = np.full(8 * 112, 0x5A, np.uint8)
    xp, op = x.ctypes.data, out.ctypes.data
    prm = lambda paths=NPATHS, per=P, md=MIN_DISTANCE, flags=0: C.byref(evplp.ProbeParams(paths, per, md, flags))     # noqa: E731
    INV = evplp.ERR_INVALID
    with evplp.Context(W, H, NPATHS, NPATHS, P, deterministic=True) as c:            # no evplp_build_accel yet
        assert L.evplp_gather_probes(c._h, prm(), xp, 8, op) == INV and b"evplp_build_accel" in L.evplp_last_error(c._h)
        assert L.evplp_gather_probes_device(c._h, prm(), xp, 8, op) == INV
        room.upload(c)
        c.upload(evplp.BUF_RECORDS, records.astype(evplp.RECORD_DTYPE))
        for form in (L.evplp_gather_probes, L.evplp_gather_probes_device):
            assert form(c._h, prm(), xp, -1, op) == INV
            assert form(c._h, prm(), None, 8, op) == INV and form(c._h, prm(), xp, 8, None) == INV
            assert form(c._h, None, xp, 8, op) == INV
            for md in (0.0, -1.0, float("nan"), float("inf")):
                assert form(c._h, prm(md=md), xp, 8, op) == INV, md
            assert form(c._h, prm(flags=1), xp, 8, op) == INV
            assert form(c._h, prm(paths=0), xp, 8, op) == INV
            assert form(c._h, prm(paths=NPATHS + 1), xp, 8, op) == INV and b"record" in L.evplp_last_error(c._h)
            assert form(c._h, prm(paths=NPATHS, per=P + 1), xp, 8, op) == INV
            assert form(c._h, prm(), xp, 0, op) == evplp.OK and form(c._h, prm(), None, 0, None) == evplp.OK      # n = 0 touches nothing
        assert (out == 0x5A).all(), "a refused call writes nothing"
        assert len(c.gather_probes(np.zeros((0, 3), F), NPATHS, P, MIN_DISTANCE)) == 0
        assert c.gather_probes(x, NPATHS, P, MIN_DISTANCE).tobytes() == base[:8].tobytes()
        # dirty vertices: refused until the refit
        c.transform_mesh(6 + 5, [1, 0, 0, 0.1, 0, 1, 0, 0, 0, 0, 1, 0])
        assert L.evplp_gather_probes(c._h, prm(), xp, 8, op) == INV and b"evplp_refit_accel" in L.evplp_last_error(c._h)
        assert (out == 0x5A).all()


# ---- 5: a moved scene
def test_a_moved_occluder_is_followed_after_the_refit(evplp, oracle, room, records, probes, ref, base):
    mesh = 6 + 5                                    # the top face of the first box: doubled and lifted under the light
    v = room.meshes[mesh]["verts"]
    centre = v.mean(0)
    target = np.array([4.2, 3.9, 3.6])
    s = 2.0
    t = target - s * centre
    m = [s, 0, 0, t[0], 0, s, 0, t[1], 0, 0, s, t[2]]
    with context(evplp, room, records) as c:
        c.transform_mesh(mesh, m)
        with pytest.raises(evplp.EvplpError) as e:
            c.gather_probes(probes, NPATHS, P, MIN_DISTANCE)
        assert e.value.status == evplp.ERR_INVALID and "evplp_refit_accel" in str(e.value)
        c.refit_accel()
        got = c.gather_probes(probes, NPATHS, P, MIN_DISTANCE)
        now = scenes.moved(room)                    # (a copy: scale 1, no offset) with the occluder where the context has it
        now.meshes[mesh]["verts"] = c.mesh_vertices(mesh, 0)
        assert not np.array_equal(now.meshes[mesh]["verts"], room.meshes[mesh]["verts"])
        now.triangle_soup()
    before = ref.lit.copy()
    try:
        ref.set_visibility(oa.Scene(now), tree=False)
        changed = int((ref.lit != before).sum())
        say(f"moved occluder: {changed} pairs changed their visibility")
        assert changed > 50
        check_values(got, ref, NPATHS, "after the refit")
        assert got.tobytes() != base.tobytes()
    finally:
        ref.set_visibility(oa.Scene(room))          # (the module's reference as it was)


# ---- 6: what the coefficients mean
def test_lambert_pixels_lit_through_their_probes_agree_with_the_vpl_gather(evplp, oracle):
    """The product's own answer: evplp_gather_vpl in mode 0 on a Lambert-only room against rho_d / pi evplp_sh_irradiance(sh, n) of probes
    at the pixels of evplp_primary.  The two differ by the order-2 expansion of the clamped cosine alone: at most
    rho_d / pi delta sum_k E_k, delta = max |A(cos) - max(cos, 0)| (about 0.09), the sum over the lit pairs in float64 -- plus the float32
    error of the two sums of at most 128 terms each, 1e-5 of the same sum."""
    w, h, n, p = 32, 24, 32, 4
    sdl = scenes.box_room(seed=7, n_boxes=4, tess=2, glossy=False, aspect=w / h)
    theta = np.linspace(0.0, np.pi, 20001)
    dirs = np.stack([np.sin(theta), np.zeros_like(theta), np.cos(theta)], -1)
    approx = ((pr.BAND * pr.basis_f64([0.0, 0.0, 1.0]))[None, :] * pr.basis_f64(dirs)).sum(-1)
    delta = float(np.abs(approx - np.maximum(np.cos(theta), 0.0)).max())
    assert 0.09 < delta < 0.1, delta
    with evplp.Context(w, h, n, n, p, deterministic=True) as c:
        sdl.upload(c)
        c.primary((0.0, 0.0), clear_light=True)
        c.trace_light_paths(3)
        c.gather_vpl(evplp.frame_params(camera_pos=sdl.cam_origin, mis_mode=0, num_light_paths=n, num_vpl_light_paths=n, photons_per_path=p))
        vpl = c.download(evplp.BUF_VPL_ACCUM)[:h].reshape(-1, 4)[:, :3].astype(np.float64)
        pos = c.download(evplp.BUF_GBUF_POSITION)[:h].reshape(-1, 4)
        nrm = c.download(evplp.BUF_GBUF_NORMAL)[:h].reshape(-1, 4)[:, :3]
        dif = c.download(evplp.BUF_GBUF_DIFFUSE)[:h].reshape(-1, 4)[:, :3].astype(np.float64)
        phg = c.download(evplp.BUF_GBUF_PHONG)[:h].reshape(-1, 4)[:, :3]
        rec = c.download(evplp.BUF_RECORDS)
        px = np.nonzero(pos[:, 3] != 0)[0]
        x = np.ascontiguousarray(pos[px, :3])
        usable = np.nonzero(rec["flags"] & 1)[0]
        d2 = ((rec["pos"][usable].astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(-1)
        min_distance = float(F(0.5 * np.sqrt(d2[d2 > 0].min())))
        assert min_distance > 1e-4, "no pixel sits on a record"
        sh = c.gather_probes(x, n, p, min_distance)
    assert (phg == 0).all() and len(px) > 0.9 * w * h, "every receiver is Lambertian (the VPLs on the light keep their emission lobe)"
    r = Reference(oa.Scene(sdl), rec.astype(oa.RECORD_DTYPE), x, min_distance, per_path=p)
    clean = ~r.aside.any(0)                     # (a pixel with a pair the oracle's tree and its brute force disagree on is set aside)
    assert r.aside_rays.sum() <= 0.005 * len(r.rays) and clean.sum() > 0.9 * len(px)
    assert np.array_equal(sh["lit"][clean], r.lit.sum(0).astype(F)[clean])
    sumE = np.where(r.lit[:, :, None], r.term[:, :, 0, :] / pr._c(0), 0.0).sum(0) / n           # term_0 = E Y0
    got = dif[px] / np.pi * np.stack([evplp.sh_irradiance(s, nn) for s, nn in zip(sh, nrm[px])]).astype(np.float64)
    bound = dif[px] / np.pi * (delta + 1e-5) * sumE
    err = np.where(clean[:, None], np.abs(got - vpl[px]), 0.0)
    say(f"meaning: {len(px)} pixels, delta {delta:.4f}, worst error / bound {float((err / np.maximum(bound, 1e-300))[bound > 0].max()):.3f}, "
        f"mean gather {vpl[px].mean():.4g}, mean |difference| {err.mean():.4g}")
    assert (err <= bound + 1e-20).all(), np.argwhere(err > bound + 1e-20)[:4]
    assert vpl[px].max() > 1e-3 and (np.abs(got - vpl[px]).sum() < 0.5 * vpl[px].sum()), "and the two are the same light, not two small numbers"
