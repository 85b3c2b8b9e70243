"""The oracle's pair shading against its float64 restatement, on inputs that visit every arm (tests/shading_domain.py).

evo_vpl_splat_pair / evo_photon_frag (and the whole-frame evo_gather_vpl / evo_splat_photons, which tile-level mistakes would show in)
are compared with vpl_pair_f64 / photon_frag_f64 on every (pixel, record, mode):
    |x - f64| <= (K 2^-24 kappa) |f64| + 1e-20        on decided pairs
K is the smallest integer that held when measured; the GPU tests (test_gpu_shading_domain.py) grant the kernels twice that.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_api as oa
import shading_domain as sd

# The smallest K that holds, measured 2026-10-18 with `pytest -s -m "not gpu" tests/test_shading_domain_host.py` (every test prints the
# worst ratio error / (2^-24 kappa |f64|) it meets), rounded up to an integer:
#   gather (evo_vpl_splat_pair = evo_gather_vpl with one slot usable): 3.24 in modes 0, 4, 5; 2.97 - 2.98 in modes 1 - 3
#   splat  (evo_photon_frag = evo_splat_photons with one photon usable): 3.38 / 2.67 / 2.66 / 2.67 / 2.65 in modes 0 - 4, 8.12 in mode 5
#          (kappa ADDS x / (x - clamp) to the conditioning of x = brdf1 brdf2 g where the two multiply; K carries the difference)
# The caps, same run: gather 1 undecided pixel under the worst record, 1 - 2 of 39839 lit pairs per mode (cap: 8, and 0.5 % = 199);
# splat 0 of 415 pairs inside the radius, no pixel within 1e-4 r of it; 37 VPL records, 24 photons.
K_ORACLE_GATHER = 4
K_ORACLE_SPLAT = 9

MODES = [0, 1, 2, 3, 4, 5]
HW = (sd.H, sd.W)


@pytest.fixture(scope="module")
def dom(oracle):
    return sd.Domain(oa)


def wi10_f32(pos):
    """normalize(cameraPosition - firstPosition) in the oracle's float32 operation order (lighttracing.cu:363)"""
    v = np.asarray(sd.CAMERA, np.float32) - pos[..., :3]
    d = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    return np.ascontiguousarray(v * (np.float32(1.0) / np.sqrt(d))[..., None], dtype=np.float32)


def test_coverage(dom):
    empty = [k for k, n in dom.coverage().items() if n == 0]
    assert not empty, empty
    assert len(dom.vpl_names) >= 36 and len(dom.photon_names) == 24


def test_floor_scene_occludes_nothing(dom):
    """rays == unoccluded pairs == the restatement's lit pairs for every record: the restatement needs no visibility"""
    fp = oa.frame_params(**sd.params(0))
    lit_any = 0
    for k, name in enumerate(dom.vpl_names):
        rays, lit = dom.oracle_scene.gather_counts(fp, sd.W, dom.gbuf, sd.only_slot(dom.vpls, k, 1), np.arange(sd.H))
        want = int(dom.vpl_ref(0, k)[4].sum())
        assert rays == lit == want, (name, rays, lit, want)
        assert (want == 0) == (name in ("facing_away", "below_floor")), (name, want)
        lit_any += want
    assert lit_any > 20000


def _gather_checks(dom, mode, images, label):
    worst, und, lit_pairs = 0.0, [], 0
    for k, name in enumerate(dom.vpl_names):
        val, kappa, lam, decided, lit = dom.vpl_ref(mode, k)
        got = images[k]
        ratio = sd.worst_ratio(got, val, kappa, lam, decided)
        worst = max(worst, ratio)
        ok = np.abs(got - val) <= sd.bar(val, kappa, lam, K_ORACLE_GATHER, False)
        bad = np.argwhere(~ok.all(-1) & decided)
        assert bad.size == 0, (label, mode, name, ratio, bad[:4].tolist(), got[tuple(bad[0])], val[tuple(bad[0])])
        assert np.all(got[~lit] == 0.0), (label, mode, name)
        if name in sd.DARK_VPLS:
            assert np.all(got == 0.0), (label, mode, name)
        und.append(int((~decided & lit).sum())); lit_pairs += int(lit.sum())
    caps = sd.check_caps(und, lit_pairs)
    print(f"\n{label} mode {mode}: worst error / (2^-24 kappa |f64|) = {worst:.2f}; undecided: worst record {caps[0]}, all {caps[1]} of {lit_pairs} lit pairs")


@pytest.mark.parametrize("mode", MODES)
def test_gather_pairs(dom, oracle, mode):
    """evo_vpl_splat_pair on every (pixel, record)"""
    fp = oa.frame_params(**sd.params(mode))
    pos, nrm, dif, phg = dom.gbuf
    wi = wi10_f32(pos)
    out = np.zeros(HW + (3,), np.float32)
    a = lambda arr: arr.ctypes.data
    fn, fpp = oracle.evo_vpl_splat_pair, C.addressof(fp)
    images = []
    for k in range(len(dom.vpl_names)):
        rec = dom.vpls[k:k + 1].copy()
        out[:] = 0.0
        rp = a(rec)
        for y, x in np.argwhere(dom.pixel.stencil):
            i = int(y) * sd.W + int(x)
            fn(fpp, a(wi) + 12 * i, a(pos) + 16 * i, a(nrm) + 16 * i, a(dif) + 16 * i, a(phg) + 16 * i, float(phg[y, x, 3]), rp, 1, a(out) + 12 * i)
        images.append(out.astype(np.float64))
    _gather_checks(dom, mode, images, "evo_vpl_splat_pair")


@pytest.mark.parametrize("mode", MODES)
def test_gather_frames(dom, mode):
    """evo_gather_vpl with one slot usable: the same bar (1 / NPATHS is exact), stencilled-out pixels untouched"""
    fp = oa.frame_params(**sd.params(mode))
    images = []
    for k in range(len(dom.vpl_names)):
        img, pairs = dom.oracle_scene.gather(fp, sd.W, sd.H, dom.gbuf, sd.only_slot(dom.vpls, k, 1))
        assert pairs == int(dom.pixel.stencil.sum())
        assert np.all(img[..., 3] == 0.0)
        images.append(img[..., :3].astype(np.float64) * sd.NPATHS)
    _gather_checks(dom, mode, images, "evo_gather_vpl")


def _splat_checks(dom, mode, images, label):
    worst, und, inside_pairs = 0.0, [], 0
    for k, name in enumerate(dom.photon_names):
        val, kappa, lam, decided, inside, rdec = dom.photon_ref(mode, k)
        assert rdec.all(), (name, "a pixel lies on the radius")
        got = images[k]
        ratio = sd.worst_ratio(got, val, kappa, lam, decided)
        worst = max(worst, ratio)
        ok = np.abs(got - val) <= sd.bar(val, kappa, lam, K_ORACLE_SPLAT, False)
        bad = np.argwhere(~ok.all(-1) & decided)
        assert bad.size == 0, (label, mode, name, ratio, bad[:4].tolist(), got[tuple(bad[0])], val[tuple(bad[0])])
        assert np.all(got[~inside] == 0.0), (label, mode, name)
        assert 8 <= inside.sum() <= 30, (name, int(inside.sum()))
        und.append(int((~decided & inside).sum())); inside_pairs += int(inside.sum())
    caps = sd.check_caps(und, inside_pairs)
    print(f"\n{label} mode {mode}: worst error / (2^-24 kappa |f64|) = {worst:.2f}; undecided: worst record {caps[0]}, all {caps[1]} of {inside_pairs} pairs")


@pytest.mark.parametrize("mode", MODES)
def test_splat_fragments(dom, oracle, mode):
    """evo_photon_frag on every (pixel, photon)"""
    fp = oa.frame_params(**sd.params(mode))
    pos, nrm, dif, phg = dom.gbuf
    a = lambda arr: arr.ctypes.data
    fn, fpp = oracle.evo_photon_frag, C.addressof(fp)
    out = np.zeros(HW + (3,), np.float32)
    images = []
    for k, s in enumerate(dom.photon_slots):
        rec = dom.photons[s - 1:s + 1].copy()
        inside = dom.photon_ref(mode, k)[4]
        out[:] = 0.0
        for i in range(sd.W * sd.H):
            kept = fn(fpp, a(rec) + 96, a(rec), a(pos) + 16 * i, a(nrm) + 16 * i, a(dif) + 16 * i, a(phg) + 16 * i, a(out) + 12 * i)
            assert not (kept and not inside.flat[i]), (dom.photon_names[k], i)
        images.append(out.astype(np.float64))
    _splat_checks(dom, mode, images, "evo_photon_frag")


@pytest.mark.parametrize("mode", MODES)
def test_splat_frames(dom, mode):
    """evo_splat_photons with one photon usable: pairs = the pixels inside the radius, the same bar"""
    fp = oa.frame_params(**sd.params(mode))
    images = []
    for k, s in enumerate(dom.photon_slots):
        img, pairs = oa.splat(fp, sd.W, sd.H, dom.gbuf, sd.only_slot(dom.photons, s, 2))
        assert pairs == int(dom.photon_ref(mode, k)[4].sum()), dom.photon_names[k]
        images.append(img[..., :3].astype(np.float64))
    _splat_checks(dom, mode, images, "evo_splat_photons")


def test_arms_are_visited(dom):
    """the inputs reach both sides of every threshold of the formulas, for some pixels of the frame and not for others"""
    lit = lambda k: dom.vpl_ref(0, k)[4]
    by = {n: k for k, n in enumerate(dom.vpl_names)}
    # the max heuristic goes both ways, the clamps of modes 4 and 5 bite and do not
    w1 = w0 = c4 = n4 = c5 = n5 = 0
    for k in range(len(dom.vpl_names)):
        v0, v2 = dom.vpl_ref(0, k)[0], dom.vpl_ref(2, k)[0]
        on = lit(k) & (v0.sum(-1) > 0)
        w1 += int((on & (v2.sum(-1) > 0)).sum()); w0 += int((on & (v2.sum(-1) == 0)).sum())
        v4, v5 = dom.vpl_ref(4, k)[0], dom.vpl_ref(5, k)[0]
        rec = dom.vpls[k]; p = dom.pixel
        d2 = ((rec["pos"].astype(np.float64) - p.pos) ** 2).sum(-1)
        g21 = np.where(on, np.maximum(rec["pos"][2] - p.pos[..., 2], 0) * np.maximum(-((rec["pos"].astype(np.float64) - p.pos) * rec["normal"]).sum(-1), 0) / d2 ** 2, 0)
        c4 += int((on & (g21 > sd.CLAMP)).sum()); n4 += int((on & (g21 < sd.CLAMP)).sum())
        flux = rec["flux"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            x5 = np.where(flux > 0, v5 / flux, 0.0)
        c5 += int((on & np.any(np.isclose(x5, np.float32(sd.CLAMP), rtol=1e-12), -1)).sum()); n5 += int((on & np.all(x5 < 0.999 * sd.CLAMP, -1)).sum())
    assert min(w1, w0, c4, n4, c5, n5) > 100, (w1, w0, c4, n4, c5, n5)
    # the lobe cut: the e = 0 VPL whose cut crosses the frame, the VPL whose lobe shows nowhere
    for name, lo, hi in (("lobe_e0_edge", 0.2, 0.8), ("lobe_away", 0.0, 0.0), ("lobe_at_frame", 0.5, 1.0)):
        k = by[name]; rec = dom.vpls[k]
        n, f = rec["normal"].astype(np.float64), rec["flux_dir"].astype(np.float64)
        v12 = rec["pos"].astype(np.float64) - dom.pixel.pos
        d = (-v12 * (2 * n * np.dot(n, f) - f)).sum(-1) / np.sqrt((v12 ** 2).sum(-1))
        frac = (d[lit(k)] > sd.CUT_CUDA).mean()
        assert lo <= frac <= hi, (name, frac)
    # splat: every MIS side and both clamps, over the photons
    s1 = s0 = b4 = f4 = b5 = f5 = 0
    for k in range(24):
        v0, v2, v4, v5 = (dom.photon_ref(m, k)[0].sum(-1) for m in (0, 2, 4, 5))
        on = v0 > 0
        s1 += int((on & (v2 > 0)).any()); s0 += int(on.any() and not (v2 > 0).any())
        b4 += int((on & (v4 > 0)).sum()); f4 += int((on & (v4 == 0)).sum()); b5 += int((on & (v5 > 0)).sum()); f5 += int((on & (v5 == 0)).sum())
    assert min(s1, s0) >= 3 and min(b4, f4, b5, f5) >= 30, (s1, s0, b4, f4, b5, f5)
    pb = {n: k for k, n in enumerate(dom.photon_names)}
    assert not dom.photon_ref(0, pb["mix_w_zero"])[0].any() and dom.photon_ref(0, pb["cc_zero"])[0].any() and not dom.photon_ref(4, pb["cc_zero"])[0].any()
    v5 = dom.photon_ref(5, pb["brdf2_zero_channel"])[0]
    assert not v5[..., 1].any() and v5[..., 0].any()
