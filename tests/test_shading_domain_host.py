"""The oracle's pair shading against its float64 restatement, on inputs that visit every arm (tests/shading_domain.py).

The VSL estimators (evo_gather_vsl, evo_vsl_splat_pair) are compared with vsl_pair_f64 on every (pixel, record, seed) under
    |x - f64| <= sum over terms of (K 2^-24 kappa_term) |term| + K 2^-24 kappa_pair |f64| + n_terms 2^-24 sum |term| + 1e-20
(shading_domain.bar_vsl); the rest of this text is about the VPL / LVC gather and the splat.

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
# The VSL estimators (evo_gather_vsl with one slot usable, against vsl_pair_f64 under bar_vsl), measured 2026-10-19 with the same command:
# worst error / (2^-24 (sum kappa_term |term| + kappa_pair |f64|)), after what K does not multiply, 0.589 under seed 11 (lambert_h0.05) and
# 0.639 (lambert_h0.001) under seed 0x9E3779B9; each estimator alone (evo_vsl_splat_pair, only = 1 / 2 / 3) 0.524 / 0.175 / 0.276.  The smallest integer that
# holds is 1: kappa_term carries the sampled direction's error in units of 2^-24 (6 - 60 of them), which the oracle's libm does not use up.
# The caps, same run: 3 undecided pixels under the worst record and 26 of 43120 lit pairs under seed 11, 2 and 13 under the other; 39 records (caps: 16, and 0.5 %).
K_ORACLE_VSL = 1

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


# ------------------------------------------------------------------------------------------------------------------ VSL
def _vsl_check(got, r, K, what, parts=None):
    """the bar on the decided pixels of one (record, seed): of the MIS-combined value, or of estimator `parts` alone"""
    val, (A, L, S, n) = (r.value, (r.A, r.L, r.S, r.n)) if parts is None else (r.parts[parts], r.part_bars[parts])
    ratio = sd.worst_ratio_vsl(got, val, A, L, S, n, r.kappa_pair, r.decided)
    ok = np.abs(got - val) <= sd.bar_vsl(val, A, L, S, n, r.kappa_pair, K, False)
    bad = np.argwhere(~ok.all(-1) & r.decided)
    assert bad.size == 0, (what, ratio, bad[:4].tolist(), got[tuple(bad[0])], val[tuple(bad[0])])
    return ratio


@pytest.mark.parametrize("seed", sd.VSL_SEEDS)
def test_vsl_per_record(dom, seed):
    """evo_gather_vsl with one slot usable against vsl_pair_f64 on every record: the bar under K_ORACLE_VSL, the exact zeros, the shaded
    stencilled-out pixels, the pair count (every pixel: no stencil test) and the caps on the undecided"""
    fp = oa.frame_params(**sd.vsl_params(seed))
    names = dom.vsl_pixel_names
    black = np.array([["black" in t for t in row] for row in names])
    off = np.array([["stencil_off_shaded" in t for t in row] for row in names])
    assert black.sum() == len(sd.VSL_BLACK_PIXELS) and off.sum() > 10 and not dom.vsl_pixel.stencil[off].any()
    worst, worst_name, und, lit_pairs, samples, off_lit, off_shaded = 0.0, "", [], 0, 0, 0, 0
    for k, name in enumerate(dom.vsl_names):
        r = dom.vsl_ref(seed, k)
        img, pairs = dom.oracle_scene.gather(fp, sd.W, sd.H, dom.vsl_gbuf, sd.only_slot(dom.vsls, k, 1), vsl=True)
        assert pairs == sd.W * sd.H, (name, pairs)
        assert np.all(img[..., 3] == 0.0)
        got = img[..., :3].astype(np.float64) * sd.NPATHS
        ratio = _vsl_check(got, r, K_ORACLE_VSL, ("evo_gather_vsl", seed, name))
        if ratio > worst: worst, worst_name = ratio, name
        assert np.all(got[~r.lit] == 0.0) and np.all(got[black] == 0.0), (seed, name)
        assert np.all(r.value[black] == 0.0) and r.lit[black].any() == r.lit.any()
        if name in sd.VSL_DARK:
            assert np.all(got == 0.0) and np.all(r.value == 0.0), (seed, name)
        else:
            shaded = off & r.lit & r.decided
            # (a lit pair may still be exactly 0 -- every cone sample of a grazing pair under c1 c2 <= 1e-9, no BRDF sample in the cone -- so:
            # non-zero wherever float64 is, and that is nearly everywhere)
            assert np.array_equal(got[shaded].sum(-1) > 0.0, r.value[shaded].sum(-1) > 0.0), (seed, name, "a stencilled-out pixel is not shaded")
            off_lit += int(shaded.sum()); off_shaded += int((got[shaded].sum(-1) > 0.0).sum())
            assert (got[shaded].sum(-1) > 0.0).any() or not shaded.any(), (seed, name)
        und.append(int((~r.decided & r.lit).sum())); lit_pairs += int(r.lit.sum())
        samples += sd.vsl_samples(r)
    caps = sd.check_caps(und, lit_pairs, per_record=16)
    print(f"\nevo_gather_vsl seed {seed:#x}: K_ORACLE_VSL measurement: worst error / (2^-24 (sum kappa |term| + kappa_pair |f64|)) = {worst:.3f} ({worst_name}); "
          f"undecided: worst record {caps[0]}, all {caps[1]} of {lit_pairs} lit pairs; {samples} sample-iterations on lit decided pairs")
    assert lit_pairs > 40000 and off_shaded > 0.95 * off_lit > 500, (off_shaded, off_lit)


def test_vsl_each_estimator_alone(dom, oracle):
    """evo_vsl_splat_pair with only = 1 / 2 / 3 (the cone, the pixel-BRDF, the VSL-BRDF estimator alone, weight 1) on a sample of pixels of
    every tile class, whole and ragged, and the black and stencilled-out pixels, against the restatement's three partial sums"""
    seed = sd.VSL_SEEDS[0]
    fp = oa.frame_params(**sd.vsl_params(seed))
    pos, nrm, dif, phg = dom.vsl_gbuf
    wi = wi10_f32(pos)
    a = lambda arr: arr.ctypes.data
    fn, fpp = oracle.evo_vsl_splat_pair, C.addressof(fp)
    pick = np.zeros(HW, bool)
    seen = set()
    for ty in range(4):
        for tx in range(6):
            key = (sd.TILES[ty][tx], ty == 3 or tx == 5)
            if key in seen:
                continue
            seen.add(key)
            for lane in (0, 9, 18, 27, 36, 45, 54, 63, 5, 58):
                y, x = ty * 8 + (lane >> 3), tx * 8 + (lane & 7)
                if y < sd.H and x < sd.W:
                    pick[y, x] = True
    for y, x in sd.VSL_BLACK_PIXELS:
        pick[y, x] = True
    pick |= np.array([["stencil_off_shaded" in t for t in row] for row in dom.vsl_pixel_names])
    assert {c for c, _ in seen} == set(sd.TILE_CLASSES) and pick.sum() > 120
    out = np.zeros(3, np.float32)
    worst = [0.0, 0.0, 0.0]; nonzero = [0, 0, 0]
    for k, name in enumerate(dom.vsl_names):
        r = dom.vsl_ref(seed, k)
        rec = dom.vsls[k:k + 1].copy()
        for only in (1, 2, 3):
            got = r.parts[only - 1].copy()          # (the pixels that are not picked compare with themselves)
            for y, x in np.argwhere(pick):
                i = int(y) * sd.W + int(x)
                fn(fpp, a(wi) + 12 * i, a(pos) + 16 * i, a(nrm) + 16 * i, a(dif) + 16 * i, a(phg) + 16 * i, float(phg[y, x, 3]), a(rec), 1,
                   i, seed, 1 + k, only, 0, a(out))
                got[y, x] = out
            worst[only - 1] = max(worst[only - 1], _vsl_check(got, r, K_ORACLE_VSL, ("evo_vsl_splat_pair", only, name), parts=only - 1))
            assert np.all(got[pick & ~r.lit] == 0.0), (only, name)
            nonzero[only - 1] += int((got[pick].sum(-1) > 0.0).sum())
    assert min(nonzero) > 100, nonzero            # (the BRDF samples hit a cone rarely: most of their pairs are 0; measured 4557 / 174 / 217)
    print(f"\nevo_vsl_splat_pair alone: worst ratio cone {worst[0]:.3f}, pixel-BRDF {worst[1]:.3f}, VSL-BRDF {worst[2]:.3f}; non-zero pairs {nonzero} of {int(pick.sum())} pixels x {len(dom.vsl_names)} records")


def test_vsl_arms_are_visited(dom):
    """the VSL inputs reach the arms the estimators have: hemispherical cones (101 samples) down to one-sample cones with 1 - cos ~ 5e-5,
    both forms of the generator's consumption rules, both lobe choices on both sides"""
    seed = sd.VSL_SEEDS[0]
    by = {n: k for k, n in enumerate(dom.vsl_names)}
    ns = np.concatenate([dom.vsl_ref(seed, k).num_samples[dom.vsl_ref(seed, k).lit] for k in range(len(dom.vsl_names))])
    assert ns.max() == 101 and ns.min() == 1 and len(np.unique(ns)) > 50
    r = dom.vsl_ref(seed, by["lambert_h50"])
    assert 1.9e4 < r.kappa_pair[r.lit].min() - 1.0 < 2.1e4 and r.num_samples.max() == 1        # 1 - cos ~ 5e-5
    hemi = [int((dom.vsl_ref(seed, k).kappa_pair[dom.vsl_ref(seed, k).lit] < 2.001).sum()) for k in range(len(dom.vsl_names))]
    assert hemi[by["lambert_h0.001"]] >= 3 and sum(hemi) >= 12, hemi      # rdratio >= 1, the hemisphere: the pixels within 0.5 of a record (0.41 apart)
    for name in ("psel_lies", "glossy_e20_p0.3", "lambert_h0.5"):   # every estimator contributes somewhere
        r = dom.vsl_ref(seed, by[name])
        assert all((p.sum(-1) > 0).sum() > 5 for p in r.parts), name
    rec = dom.vsls[by["psel_lies"]]
    true = rec["rho_d"].max() / (rec["rho_d"].max() + rec["rho_s"].max())
    assert abs(float(rec["p_select_lambert"]) - float(true)) > 0.2
