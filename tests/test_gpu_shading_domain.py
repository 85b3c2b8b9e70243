"""The shading of the VPL / LVC gather and of the photon splat against float64, over the material domain (tests/shading_domain.py).

Per record and per MIS / clamp mode, gather_vpl (entry cuts on and off), gather_lvc and splat_photons run with ONE record usable over the
44 x 28 floor G-buffer whose tiles carry every material class, and every decided pixel is compared with the float64 restatement:
    |x - f64| <= (K 2^-24 kappa + 2^-22 lam) |f64| + 1e-20
K = 2 x the K measured for the fp32 oracle (test_shading_domain_host.py): the kernels take 1-ulp rsq / rcp where the oracle has
correctly rounded sqrt and division, so each rounding may double; the lam term is the stated bound of exp2(e log2 d) on the hardware
transcendentals, which both vpl_shade (kernels_gather.hip:41-50) and the splat (kernels_splat.hip:37-44, pow_hw) use.  Undecided
pixels (a discrete comparison within its margin) are compared with nothing; the host test caps how many there are.

Measured on an MI355X, 2026-10-18 (`pytest -s -m gpu tests/test_gpu_shading_domain.py` prints them), error / bar at its worst:
gather_vpl, gather_lvc and gather_vpl from the root 0.343 - 0.344 in every mode (K = 8); the whole set 0.306 - 0.311; splat_photons 0.180 /
0.148 / 0.147 / 0.148 / 0.147 / 0.246 in modes 0 - 5 (K = 18).

The VSL gather (gather_vsl_walk_kernel + gather_vsl_shade_kernel) runs the same way over the domain's VSL inputs -- the receiver without its
stencil and with four black pixels, two more records, vsl_radius 0.5, two seeds -- against vsl_pair_f64 under shading_domain.bar_vsl:
    |x - f64| <= sum over terms of (K 2^-24 kappa_term + 2^-22 lam_term) |term| + K 2^-24 kappa_pair |f64| + n_terms 2^-24 sum |term| + 1e-20
with K = 2 x K_ORACLE_VSL = 2.  kappa_term carries the sampled direction's error, whose hardware part (v_sin / v_cos, the Phong samples' cos_t)
is what evplp_selftest(4) measures (test_gpu_parity.py::test_hardware_primitives_of_the_vsl_estimators): 1.254e-7 / 1.254e-7 / 7.23e-8
absolute, rcp / rsq / sqrt 9.13e-8 / 9.38e-8 / 9.27e-8 relative on an MI355X, 2026-10-19.  Measured the same day, error / bar at its worst:
per record 0.371 (seed 11) and 0.411 (seed 0x9E3779B9); Lambert pixels under Lambert records 0.362 / 0.356 in lambert tiles (the
estimators' wave-uniform diffuse form) and 0.357 / 0.375 in tiles with one glossy lane (the general form); from the root 0.371; the whole
set 0.230 with 97.9 % of the pixels decided under all 39 records.  A deliberately wrong estimator fails test_gather_vsl_per_record by
these factors of the bar: pdf2's Phong term times (1 - L.psel) 3.7e3 (1017 pixels), P.glossy for P.pdf_glossy 25 (the rsx_zero pixels under
the Lambert records closest to the floor), the diffuse form's cone sample without 1 / solid angle 1.7e7; the oracle comparison at 1e-3 / 2 %
(test_gpu_parity.py, test_gpu_leaf_step.py) sees only the last of the three.
"""
import numpy as np
import pytest

import oracle_api as oa
import shading_domain as sd
from test_shading_domain_host import K_ORACLE_GATHER, K_ORACLE_SPLAT, K_ORACLE_VSL

pytestmark = pytest.mark.gpu

K_GPU_GATHER = 2 * K_ORACLE_GATHER
K_GPU_SPLAT = 2 * K_ORACLE_SPLAT
K_GPU_VSL = 2 * K_ORACLE_VSL
MODES = [0, 1, 2, 3, 4, 5]
W, H = sd.W, sd.H


@pytest.fixture(scope="module")
def dom(oracle):
    d = sd.Domain(oa)
    empty = [k for k, n in d.coverage().items() if n == 0]
    assert not empty, empty
    fp = oa.frame_params(**sd.params(0))
    d.counts = [d.oracle_scene.gather_counts(fp, W, d.gbuf, sd.only_slot(d.vpls, k, 1), np.arange(H)) for k in range(len(d.vpl_names))]
    return d


def make_context(evplp, dom, gbuf=None, **kw):
    c = evplp.Context(W, H, sd.NPATHS, sd.NPATHS, sd.P, bvh_builder=evplp.BVH_SAH, deterministic=True, **kw)
    dom.scene.upload(c)
    c.primary((0.0, 0.0))                           # (the splat projects photons through the camera of the frame)
    for b, plane in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG), dom.gbuf if gbuf is None else gbuf):
        pad = np.zeros((c.local_rows, W, 4), np.float32); pad[:H] = plane
        c.upload(b, pad)
    return c


def compare(got, ref, K, what):
    """the bar on the decided pixels; returns error / bar at its worst"""
    val, kappa, lam, decided = ref[:4]
    got = got.astype(np.float64)
    assert np.isfinite(got).all(), what
    b = sd.bar(val, kappa, lam, K, True)
    ratio = np.where(decided[..., None], np.abs(got - val) / b, 0.0)
    worst = float(ratio.max())
    if worst > 1.0:
        y, x, ch = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: pixel ({x}, {y}) channel {ch}: got {got[y, x, ch]!r}, float64 {val[y, x, ch]!r}, error / bar {worst:.3g}, "
                             f"kappa {np.broadcast_to(kappa if kappa.ndim == 3 else kappa[..., None], val.shape)[y, x, ch]:.4g}, lam {lam[y, x]:.4g}; "
                             f"{int((ratio > 1).any(-1).sum())} pixels outside")
    return worst


def run_gather_per_record(evplp, dom, mode, lvc):
    worst = 0.0
    fp = evplp.frame_params(**sd.params(mode), rng_seed=11)
    which = evplp.PASS_GATHER_LVC if lvc else evplp.PASS_GATHER_VPL
    with make_context(evplp, dom) as c:
        for k, name in enumerate(dom.vpl_names):
            c.upload(evplp.BUF_RECORDS, sd.only_slot(dom.vpls, k, 1))
            c.clear_accumulators()
            (c.gather_lvc if lvc else c.gather_vpl)(fp)
            got = c.download(evplp.BUF_VPL_ACCUM)[:H]
            st = c.pass_stats(which)
            val, kappa, lam, decided, lit = dom.vpl_ref(mode, k)
            what = f"{'gather_lvc' if lvc else 'gather_vpl'} mode {mode} record {name}"
            if lvc:     # (this pass counts evaluated pairs and shadow rays only)
                assert (st["pairs"], st["rays"]) == (int(dom.pixel.stencil.sum()), dom.counts[k][0]), (what, st["pairs"], st["rays"], dom.counts[k])
            else:
                assert st["usable"] == 1, what
                assert (st["rays"], st["shaded"]) == dom.counts[k], (what, st["rays"], st["shaded"], dom.counts[k])
            assert np.all(got[~dom.pixel.stencil] == 0.0), what + ": a stencilled-out pixel was written"
            assert np.all(got[..., :3][~lit] == 0.0), what + ": an unlit pair contributes"
            if name in sd.DARK_VPLS:
                assert np.all(got == 0.0), what
            worst = max(worst, compare(got[..., :3] * np.float32(sd.NPATHS), (val, kappa, lam, decided), K_GPU_GATHER, what))
    return worst


@pytest.mark.parametrize("mode", MODES)
def test_gather_vpl_per_record(evplp, dom, monkeypatch, mode):
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    worst = run_gather_per_record(evplp, dom, mode, lvc=False)
    print(f"\ngather_vpl mode {mode}: worst error / bar {worst:.3f} (K = {K_GPU_GATHER})")


@pytest.mark.parametrize("mode", MODES)
def test_gather_lvc_per_record(evplp, dom, monkeypatch, mode):
    """the window of numVplLightPaths = numLightPaths paths holds every path whatever the pixel's offset"""
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    worst = run_gather_per_record(evplp, dom, mode, lvc=True)
    print(f"\ngather_lvc mode {mode}: worst error / bar {worst:.3f} (K = {K_GPU_GATHER})")


@pytest.mark.parametrize("mode", [0, 3, 5])
def test_gather_vpl_from_the_root(evplp, dom, monkeypatch, mode):
    """gather_vpl_kernel<false>: no entry cuts, every walk from the root (EVPLP_CUTS is read when the context is created)"""
    monkeypatch.setenv("EVPLP_CUTS", "0")
    worst = run_gather_per_record(evplp, dom, mode, lvc=False)
    print(f"\ngather_vpl from the root, mode {mode}: worst error / bar {worst:.3f} (K = {K_GPU_GATHER})")


@pytest.mark.parametrize("mode", MODES)
def test_gather_whole_set(evplp, dom, monkeypatch, mode):
    """every record usable at once, against the float64 sum; twice with doAccumulate = 1.  The bar of a sum: the bars of its terms, and
    2^-24 of the running sum (at most the sum of magnitudes) for each of its additions."""
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    n = len(dom.vpl_names)
    refs = [dom.vpl_ref(mode, k) for k in range(n)]
    total = sum(r[0] for r in refs)
    bars = sum(sd.bar(r[0], r[1], r[2], K_GPU_GATHER, True) for r in refs) + n * 2.0 ** -24 * sum(np.abs(r[0]) for r in refs)
    decided = np.logical_and.reduce([r[3] for r in refs])
    assert decided.mean() > 0.98
    fp = evplp.frame_params(**sd.params(mode, do_accumulate=1))
    with make_context(evplp, dom) as c:
        c.upload(evplp.BUF_RECORDS, dom.vpls)
        c.clear_accumulators()
        c.gather_vpl(fp)
        once = c.download(evplp.BUF_VPL_ACCUM)[:H]
        st = c.pass_stats(evplp.PASS_GATHER_VPL)
        c.gather_vpl(fp)
        twice = c.download(evplp.BUF_VPL_ACCUM)[:H]
    assert st["usable"] == n
    assert (st["rays"], st["shaded"]) == (sum(r for r, _ in dom.counts), sum(s for _, s in dom.counts))
    assert np.all(once[~dom.pixel.stencil] == 0.0) and np.all(twice[~dom.pixel.stencil] == 0.0)
    worst = 0.0
    for times, got in ((1, once), (2, twice)):
        ratio = np.where(decided[..., None], np.abs(got[..., :3].astype(np.float64) * sd.NPATHS - times * total) / (times * bars), 0.0)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (mode, times, np.unravel_index(int(ratio.argmax()), ratio.shape), float(ratio.max()))
    print(f"\ngather_vpl whole set, mode {mode}: worst error / bar {worst:.3f}")


@pytest.mark.parametrize("mode", MODES)
def test_splat_per_photon(evplp, dom, monkeypatch, mode):
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    fp = evplp.frame_params(**sd.params(mode))
    worst = 0.0
    with make_context(evplp, dom) as c:
        for k, (name, s) in enumerate(zip(dom.photon_names, dom.photon_slots)):
            c.upload(evplp.BUF_RECORDS, sd.only_slot(dom.photons, s, 2))
            c.splat_photons(fp, clear=True)
            got = c.download(evplp.BUF_PHOTON_ACCUM)[:H]
            st = c.pass_stats(evplp.PASS_SPLAT)
            val, kappa, lam, decided, inside, rdec = dom.photon_ref(mode, k)
            what = f"splat_photons mode {mode} photon {name}"
            assert rdec.all(), what
            assert st["pairs"] == int(inside.sum()), (what, st["pairs"], int(inside.sum()))
            assert np.all(got[..., :3][~inside] == 0.0), what + ": a pixel outside the radius was written"
            worst = max(worst, compare(got[..., :3], (val, kappa, lam, decided), K_GPU_SPLAT, what))
    print(f"\nsplat_photons mode {mode}: worst error / bar {worst:.3f} (K = {K_GPU_SPLAT})")


# ------------------------------------------------------------------------------------------------------------------ VSL
def vsl_ratio(got, r, K):
    """error / bar_vsl per channel, 0 on the undecided pixels"""
    b = sd.bar_vsl(r.value, r.A, r.L, r.S, r.n, r.kappa_pair, K, True)
    return np.where(r.decided[..., None], np.abs(got.astype(np.float64) - r.value) / b, 0.0)


def tags(dom, tag):
    return np.array([[tag in t for t in row] for row in dom.vsl_pixel_names])


def tile_mask(classes):
    return np.array([[sd.TILES[y >> 3][x >> 3] in classes for x in range(W)] for y in range(H)])


def run_gather_vsl_per_record(evplp, dom, seed):
    """-> error / bar at its worst: over everything, over the Lambert pixels of `lambert` tiles under Lambert records (the estimators' wave-uniform
    diffuse form), over the Lambert pixels of one_lane0 / one_mid / one_lane63 tiles under the same records (one glossy lane: the general form)"""
    fp = evplp.frame_params(**sd.vsl_params(seed))
    black, off = tags(dom, "black"), tags(dom, "stencil_off_shaded")
    lambert_px = tags(dom, "lambert_e_left") & ~black
    form_diffuse, form_general = lambert_px & tile_mask(("lambert",)), lambert_px & tile_mask(("one_lane0", "one_mid", "one_lane63"))
    assert form_diffuse.sum() > 200 and form_general.sum() > 200
    worst = [0.0, 0.0, 0.0]
    exact = 0
    with make_context(evplp, dom, dom.vsl_gbuf) as c:
        for k, name in enumerate(dom.vsl_names):
            c.upload(evplp.BUF_RECORDS, sd.only_slot(dom.vsls, k, 1))
            c.clear_accumulators()
            c.gather_vsl(fp)
            got = c.download(evplp.BUF_VPL_ACCUM)[:H]
            st = c.pass_stats(evplp.PASS_GATHER_VSL)
            r = dom.vsl_ref(seed, k)
            what = f"gather_vsl seed {seed:#x} record {name}"
            assert np.isfinite(got).all(), what
            assert st["usable"] == 1 and st["pairs"] == W * H, (what, st["usable"], st["pairs"])
            if r.decided.all():         # (then the lit pairs are the restatement's, every one of them)
                assert (st["rays"], st["samples"]) == (int(r.lit.sum()), sd.vsl_samples(r)), (what, st["rays"], st["samples"], int(r.lit.sum()), sd.vsl_samples(r))
                exact += 1
            val = got[..., :3] * np.float32(sd.NPATHS)
            assert np.all(val[~r.lit & r.decided] == 0.0), what + ": an unlit pair contributes"
            assert np.all(val[black] == 0.0), what + ": a black pixel was shaded"
            if name in sd.VSL_DARK:
                assert np.all(got == 0.0), what
            shaded = off & r.lit & r.decided
            assert np.array_equal(val[shaded].sum(-1) > 0.0, r.value[shaded].sum(-1) > 0.0), what + ": a stencilled-out pixel is not shaded as float64 has it"
            ratio = vsl_ratio(val, r, K_GPU_VSL)
            if ratio.max() > 1.0:
                y, x, ch = np.unravel_index(int(ratio.argmax()), ratio.shape)
                raise AssertionError(f"{what}: pixel ({x}, {y}) channel {ch} ({dom.vsl_pixel_names[y, x]}, tile {sd.TILES[y >> 3][x >> 3]}): got {val[y, x, ch]!r}, "
                                     f"float64 {r.value[y, x, ch]!r}, error / bar {ratio.max():.3g}, {r.num_samples[y, x]} samples; {int((ratio > 1).any(-1).sum())} pixels outside")
            worst[0] = max(worst[0], float(ratio.max()))
            if not np.any(dom.vsls[k]["rho_s"] != 0.0):
                worst[1] = max(worst[1], float(ratio[form_diffuse].max())); worst[2] = max(worst[2], float(ratio[form_general].max()))
    assert exact >= len(dom.vsl_names) // 3, exact        # (the statistics were compared exactly under that many records)
    return worst


@pytest.mark.parametrize("seed", sd.VSL_SEEDS)
def test_gather_vsl_per_record(evplp, dom, monkeypatch, seed):
    """One slot usable (the usable slot sits behind a gap of unusable ones: the stream's key is the slot, vpl_src_index, not the compacted
    index), against vsl_pair_f64: the bar on the decided pixels, the exact zeros, the shaded stencilled-out pixels, the statistics"""
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    worst = run_gather_vsl_per_record(evplp, dom, seed)
    print(f"\ngather_vsl seed {seed:#x}: worst error / bar {worst[0]:.3f} (K = {K_GPU_VSL}); Lambert pixels under Lambert records: "
          f"diffuse form (lambert tiles) {worst[1]:.3f}, general form (one glossy lane in the tile) {worst[2]:.3f}")


def test_gather_vsl_from_the_root(evplp, dom, monkeypatch):
    """gather_vsl_walk_kernel<false>: no entry cuts, every walk from the root (EVPLP_CUTS is read when the context is created)"""
    monkeypatch.setenv("EVPLP_CUTS", "0")
    worst = run_gather_vsl_per_record(evplp, dom, sd.VSL_SEEDS[0])
    print(f"\ngather_vsl from the root: worst error / bar {worst[0]:.3f} (K = {K_GPU_VSL}); diffuse form {worst[1]:.3f}, general form {worst[2]:.3f}")


def test_gather_vsl_whole_set(evplp, dom, monkeypatch):
    """every record usable at once, against the float64 sum, once and twice with doAccumulate = 1; the image is the same bytes for 1, 2 and 8
    splits per wave.  The bar of a sum: the bars of its terms, and 2^-24 of the running sum for each of its additions."""
    monkeypatch.delenv("EVPLP_CUTS", raising=False)
    seed = sd.VSL_SEEDS[0]
    n = len(dom.vsl_names)
    refs = [dom.vsl_ref(seed, k) for k in range(n)]
    total = sum(r.value for r in refs)
    bars = sum(sd.bar_vsl(r.value, r.A, r.L, r.S, r.n, r.kappa_pair, K_GPU_VSL, True) for r in refs) + n * 2.0 ** -24 * sum(np.abs(r.value) for r in refs)
    decided = np.logical_and.reduce([r.decided for r in refs])
    # the caps of the host test: at most 0.5 % of the lit pairs are undecided, each takes one pixel out of the intersection at the most
    floor = 1.0 - 0.005 * sum(int(r.lit.sum()) for r in refs) / (W * H)
    assert decided.mean() > floor > 0.8, (decided.mean(), floor)
    fp = evplp.frame_params(**sd.vsl_params(seed, do_accumulate=1))
    images = {}
    for k in (1, 2, 8):
        with make_context(evplp, dom, dom.vsl_gbuf, gather_splits_per_wave=k) as c:
            c.upload(evplp.BUF_RECORDS, dom.vsls)
            c.clear_accumulators()
            c.gather_vsl(fp)
            images[k] = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
            if k == 1:
                st = c.pass_stats(evplp.PASS_GATHER_VSL)
                c.gather_vsl(fp)
                twice = c.download(evplp.BUF_VPL_ACCUM)[:H].copy()
    assert images[2].tobytes() == images[1].tobytes() and images[8].tobytes() == images[1].tobytes(), "the image depends on the splits per wave"
    assert st["usable"] == n and st["pairs"] == W * H * n
    if all(r.decided.all() for r in refs):
        assert (st["rays"], st["samples"]) == (sum(int(r.lit.sum()) for r in refs), sum(sd.vsl_samples(r) for r in refs))
    worst = 0.0
    for times, got in ((1, images[1]), (2, twice)):
        assert np.isfinite(got).all() and np.all(got[..., 3] == 0.0)
        ratio = np.where(decided[..., None], np.abs(got[..., :3].astype(np.float64) * sd.NPATHS - times * total) / (times * bars), 0.0)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (times, np.unravel_index(int(ratio.argmax()), ratio.shape), float(ratio.max()))
    print(f"\ngather_vsl whole set: worst error / bar {worst:.3f}; decided {decided.mean():.4f} (floor {floor:.3f})")
