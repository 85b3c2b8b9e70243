"""The oracle's light tracing and path tracer against their float64 restatement, on inputs that visit every arm (tests/feeder_domain.py).

evo_trace_light_paths is compared vertex by vertex (feeder_domain.light_path_f64, teacher-forced from the records under test): flags, the
untextured triangle's material and the zeroed tail exactly; positions, normals, directions, psel, texels and flux under
    |x - f64| <= K 2^-24 kappa scale + 1e-20
with scale = |f64| per component for psel, texels and flux, 1 for unit vectors and (largest coordinate of the ray's origin + t) for
positions -- a component near zero of a vector is not known to a relative 2^-24 of itself.
evo_path_trace is compared per pixel (feeder_domain.path_pixel_f64) under
    |x - f64| <= K 2^-24 sum kappa_term |term| + n_terms 2^-24 sum |term| + 1e-20
on decided pixels; undecided ones are compared with nothing and counted against the cap of 1 % per case.
K is the smallest integer that held when measured; the GPU tests (test_gpu_feeder_domain.py) grant the kernels twice that.
"""
from collections import Counter

import numpy as np
import pytest

import feeder_domain as fd
import oracle_api as oa

# The smallest K that holds, measured 2026-10-21 with `pytest -s -m "not gpu" tests/test_feeder_domain_host.py` (every test prints the worst
# ratio it meets), rounded up to an integer:
#   light tracing, error / (2^-24 kappa scale): 0.51 - 0.53 under seed 0x68 and 0.53 - 0.74 under 0x9e3779cd with light exponent 0, 0.37 - 0.43
#                  and 0.42 - 0.70 with exponent 5, over P = 2, 4, 7 (a hit position or the direction leaving a vertex)
#   path tracer, error / (2^-24 sum kappa |term|) after what K does not multiply: uploaded receiver, one sample 0.83 - 0.95 (exponent 0) and
#                  1.19 - 1.27 (exponent 5) over 1, 2, 3 bounces; two accumulated samples 0.71 - 0.86; the scene's own primary G-buffer
#                  (what the batched call draws), two samples, 0.43 / 0.76
# The caps, same run: light tracing 0 - 2 undecided of 200 paths per case (cap 2); path tracer 1 - 3 undecided of 1208 stencilled pixels per
# single sample, 1 - 6 for two accumulated samples, 8 of 1232 in the primary view (cap 12).  Coverage, same run, decided samples only: the
# light's small triangle drawn 5 and 6 times in 200 paths under the two seeds, 226 times in the path tracer; the rarest arms are
# tex_u_above_1 (5), tex_v_below_0 (12), lt_first:e_1 (18) in light tracing and pt_emitter_from_phong (32), tex_u_below_0 (42) in the path tracer.
# A kappa that lacked the cosine of incidence under a hit's displacement, or the incoming direction's error under a mirrored sample, showed
# as 10 - 11 here in the primary view (a grazing hit on a wall after an e = 200 lobe): those two terms are in feeder_domain.path_pixel_f64.
K_ORACLE_LT = 1
K_ORACLE_PT = 2

CAP = 0.01
LT_CASES = [(e, P) for e in fd.LIGHT_EXPONENTS for P in fd.LT_P]
PT_CASES = [(e, b) for e in fd.LIGHT_EXPONENTS for b in fd.PT_BOUNCES]


@pytest.fixture(scope="module")
def dom(oracle):
    d = fd.Domain(oa)
    d.oracle_scenes = {e: oa.Scene(s) for e, s in d.scenes.items()}
    return d


def big_records(n):
    """n record slots that hold 1e30 in every word: a slot the tracer does not write shows"""
    return np.full(n * 24, fd.BIG, np.float32).view(oa.RECORD_DTYPE)


def check_lt(r, K, what):
    assert not r.exact, (what, len(r.exact), r.exact[:3])
    assert r.worst <= K, (what, r.worst, r.worst_what)
    assert r.undecided <= CAP * r.paths, (what, r.undecided, r.paths)


def check_pt(got, ref, K, what):
    """the bar on the decided pixels, exact zeros where the stencil is off, the cap; returns (error / bar at its worst, undecided pixels)"""
    assert np.isfinite(got).all(), what
    ratio, (x, y, c) = fd.path_worst_ratio(got[..., :3], ref)
    assert ratio <= K, f"{what}: pixel ({x}, {y}) channel {c}: got {got[y, x, c]!r}, float64 {ref.value[y, x, c]!r}, error / (2^-24 sum kappa |term|) = {ratio:.3g}"
    und = int((~ref.decided & ref.stencil).sum())
    assert und <= CAP * int(ref.stencil.sum()), (what, und)
    return ratio / K, und


def test_generator_restatement(oracle):
    """the integer restatement of the stream against the oracle's generator, whose first words test_rng_known_answers pins"""
    import ctypes as C
    for index, seq, sub in ((0, 0, 0), (199, 104, 0), (7, 0x9E3779CD, 0), (27 * fd.W + 43, 4, fd.PT_SUBSTREAM), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
        r = oa.Rng()
        oracle.evo_rng_init(C.byref(r), index, seq, sub)
        u32 = fd.stream(index, seq, sub)
        assert [oracle.evo_rng_u32(C.byref(r)) for _ in range(8)] == [u32() for _ in range(8)], (index, seq, sub)
        oracle.evo_rng_init(C.byref(r), index, seq, sub)
        u = fd.uniforms(index, seq, sub)
        assert [float(oracle.evo_rng_uniform(C.byref(r))) for _ in range(8)] == [u() for _ in range(8)]


def test_scene_is_what_the_header_says(dom):
    for e, G in dom.geo.items():
        assert 40 <= len(G.mat) <= 70 and G.light_count == 3 and G.lw == e
        areas = np.diff(np.concatenate([[0.0], G.cdf])) * G.light_area
        assert areas[2] < 0.01 * G.light_area and areas[0] > 1.9 * areas[1] > 50 * areas[2]
        assert abs(dom.oracle_scenes[e].lib.evo_scene_light_area(dom.oracle_scenes[e].h) - G.light_area) < 1e-6 * G.light_area
        assert sorted(t.shape[:2] for t in G.textures) == [(1, 1), (3, 5), (3, 5)]
        assert {"black", "back", "textured", "light"} <= set(G.cls) and set(fd.CLASSES) <= set(G.cls)
        assert np.all(G.p0[G.light_first:G.light_first + 3, 2] == 0.0)
    # the receiver: shading_domain's ragged frame and tile layout
    assert dom.gbuf[0].shape == (fd.H, fd.W, 4) and 0 < int((~dom.stencil).sum()) < 40
    assert np.all(dom.gbuf[2][~dom.stencil][:, :3] == fd.BIG)


@pytest.fixture(scope="module")
def lt_results(dom):
    out = {}
    for e, P in LT_CASES:
        for seed in fd.LT_SEEDS:
            rec = dom.oracle_scenes[e].trace_light_paths(seed, fd.LT_PATHS, P, records=big_records(fd.LT_PATHS * P))
            out[e, P, seed] = (rec, fd.check_light_paths(dom.geo[e], rec, seed, P))
    return out


@pytest.mark.parametrize("e, P", LT_CASES)
def test_light_paths(lt_results, e, P):
    for seed in fd.LT_SEEDS:
        rec, r = lt_results[e, P, seed]
        check_lt(r, K_ORACLE_LT, (e, P, seed))
        assert r.compared > 10 * fd.LT_PATHS
        print(f"\nlight tracing, exponent {e:g}, P = {P}, seed {seed:#x}: worst error / (2^-24 kappa scale) = {r.worst:.2f} ({r.worst_what.split(':')[0]}); "
              f"{r.undecided} undecided of {r.paths} paths; {r.compared} comparisons")


def test_light_paths_coverage(lt_results):
    cov = sum((r.coverage for _, r in lt_results.values()), Counter())
    fd.check_arms(cov, fd.LT_ARMS)
    per_seed = {seed: lt_results[5.0, 2, seed][1].coverage["light_triangle_2"] for seed in fd.LT_SEEDS}
    assert min(per_seed.values()) >= 3, per_seed
    print("\nlight tracing coverage:", sorted(cov.items()))


def test_a_perturbed_restatement_is_caught(dom, lt_results):
    """the comparison can fail: beta and gamma swapped on the light, and the stored flux taken after the division by the roulette
    probability, each leave decided vertices far outside the bar"""
    rec, r = lt_results[5.0, 4, fd.LT_SEEDS[0]]
    assert r.worst <= K_ORACLE_LT
    for perturb, where in (("swap_beta_gamma", "on-light position"), ("flux_after_division", "flux")):
        bad = fd.check_light_paths(dom.geo[5.0], rec, fd.LT_SEEDS[0], 4, perturb=perturb)
        assert bad.worst > 1000.0 * K_ORACLE_LT and where in bad.worst_what, (perturb, bad.worst, bad.worst_what)
        print(f"\n{perturb}: error / (2^-24 kappa scale) = {bad.worst:.3g} at {bad.worst_what.split(':')[0]}")


@pytest.mark.parametrize("e, bounces", PT_CASES)
def test_path_trace(dom, e, bounces):
    """one sample written over a dirty accumulator, then two accumulated from a clear one"""
    osc, s0, s1 = dom.oracle_scenes[e], *fd.PT_SEEDS
    n_stencil = int(dom.stencil.sum())
    ref = dom.pt_ref(e, s0, bounces)
    out = np.full((fd.H, fd.W, 4), 7.0, np.float32)
    got, n = osc.path_trace(fd.CAMERA, s0, bounces, fd.W, fd.H, dom.gbuf, out=out, accumulate=False)
    assert n == n_stencil and np.all(got[~dom.stencil] == 7.0)
    worst, und = check_pt(got, ref, K_ORACLE_PT, ("single", e, bounces))
    got, _ = osc.path_trace(fd.CAMERA, s0, bounces, fd.W, fd.H, dom.gbuf)
    got, _ = osc.path_trace(fd.CAMERA, s1, bounces, fd.W, fd.H, dom.gbuf, out=got)
    assert np.all(got[~dom.stencil] == 0.0)
    both = fd.add_images(ref, dom.pt_ref(e, s1, bounces))
    worst2, und2 = check_pt(got, both, K_ORACLE_PT, ("accumulated", e, bounces))
    assert int(ref.rays[dom.stencil].min()) >= 1 and int(ref.rays.max()) <= 1 + 2 * bounces
    print(f"\npath tracer, exponent {e:g}, {bounces} bounces: error / bar {worst:.3f} (one sample), {worst2:.3f} (two); undecided {und} and {und2} of {n_stencil}")


def test_path_trace_primary_view(dom):
    """the G-buffer the batched call draws for itself: the scene's own camera, textured and emitting pixels included"""
    for e, osc in dom.oracle_scenes.items():
        cam = dom.scenes[e].cam_origin
        gbuf = osc.primary(fd.W, fd.H, (0.0, 0.0))[:4]
        ref = fd.add_images(*[fd.path_image_f64(dom.geo[e], gbuf, None, cam, s, 3) for s in fd.PT_SEEDS])
        got, n = osc.path_trace(cam, fd.PT_SEEDS[0], 3, fd.W, fd.H, gbuf)
        got, n = osc.path_trace(cam, fd.PT_SEEDS[1], 3, fd.W, fd.H, gbuf, out=got)
        worst, und = check_pt(got, ref, K_ORACLE_PT, ("primary view", e))
        print(f"\npath tracer on the primary view, exponent {e:g}, two samples: error / bar {worst:.3f}; undecided {und} of {n}")


def test_path_trace_coverage(dom):
    cov = sum((dom.pt_ref(e, s, b).cov for e, b in PT_CASES for s in fd.PT_SEEDS), Counter())
    fd.check_arms(cov, fd.PT_ARMS)
    print("\npath tracer coverage:", sorted(cov.items()))
