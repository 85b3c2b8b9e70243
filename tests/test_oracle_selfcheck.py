"""Self-consistency of the CPU oracle (no GPU): its BVH against brute force, RNG known answers, BRDF
identities, energy conservation of light tracing, the progressive schedule."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_api as oa
import scenes
from shading_domain import vsl_stream as _vsl_stream     # the estimators' generator restated in integers, beside its vectorised form


@pytest.fixture(scope="module")
def room_scene():
    room = scenes.box_room(seed=11, n_boxes=6, tess=2, textured=True)
    return room, oa.Scene(room)


def test_record_layout_is_96_bytes():
    assert oa.RECORD_DTYPE.itemsize == 96                      # rtphotonrecord.h:17-25
    assert oa.RECORD_DTYPE.fields["flags"][1] == 12 and oa.RECORD_DTYPE.fields["phong_exp"][1] == 92


def test_rng_known_answers(oracle):
    r = oa.Rng()
    oracle.evo_rng_init(C.byref(r), 0, 0, 0)
    first = [oracle.evo_rng_u32(C.byref(r)) for _ in range(4)]
    oracle.evo_rng_init(C.byref(r), 0, 0, 0)
    assert first == [oracle.evo_rng_u32(C.byref(r)) for _ in range(4)]
    # pure-python restatement of the generator (splitmix64 + PCG32 XSH-RR)
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    def stream(index, seq, sub, n):
        s0 = sm((((seq << 32) | index) + sub * 0xD1B54A32D192ED03) & M)
        inc = sm(s0) | 1
        state = (s0 + inc) & M
        out = []
        for k in range(n + 1):
            old = state
            state = (old * 6364136223846793005 + inc) & M
            xs = (((old >> 18) ^ old) >> 27) & 0xFFFFFFFF
            rot = old >> 59
            out.append(((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF)
        return out[1:]
    for index, seq, sub in ((0, 0, 0), (7, 3, 0), (123456, 99, 17)):
        oracle.evo_rng_init(C.byref(r), index, seq, sub)
        got = [oracle.evo_rng_u32(C.byref(r)) for _ in range(5)]
        assert got == stream(index, seq, sub, 5)
    oracle.evo_rng_init(C.byref(r), 1, 2, 3)
    u = np.array([oracle.evo_rng_uniform(C.byref(r)) for _ in range(20000)])
    assert u.min() > 0.0 and u.max() <= 1.0 and abs(u.mean() - 0.5) < 0.01      # (0,1] like curand_uniform


def test_vsl_rng_known_answers_and_statistics(oracle):
    """The VSL estimators' stream: state words equal to a pure-python xoroshiro64, the three draws of a step served in the reference's
    order (lobe choice from the 16 left-over bits, then the two 24-bit uniforms), and -- because the generator is the build's own
    choice -- chi-square checks of what the estimators rely on: uniform marginals, the two uniforms of a sample independent of each
    other and of the neighbouring samples', streams of neighbouring records and pixels independent at every early step."""
    r = oa.Rng()
    for index, seq, sub in ((0, 0, 1), (7, 3, 2), (123456, 99, 17), (2047 * 2048, 0xFFFFFFFF, 16384)):
        oracle.evo_vsl_rng_init(C.byref(r), index, seq, sub)
        for s0, s1 in _vsl_stream(index, seq, sub, 6):
            oracle.evo_vsl_rng_step(C.byref(r))
            assert (r.s0, r.s1) == (s0, s1)
            draws = [oracle.evo_rng_uniform(C.byref(r)) for _ in range(3)]
            assert draws == [np.float32((((s0 & 0xFF) << 8 | (s1 & 0xFF)) + 0.5) / 65536.0), np.float32(((s0 >> 8) + 1) / 16777216.0),
                             np.float32(((s1 >> 8) + 1) / 16777216.0)]
    # statistics, vectorised restatement (checked against the scalar one first)
    U = np.uint64
    M32 = U(0xFFFFFFFF)

    def sm(x):
        with np.errstate(over="ignore"):
            x = x + U(0x9E3779B97F4A7C15)
            x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
            return x ^ (x >> U(31))
    rotl = lambda x, k: ((x << U(k)) | (x >> U(32 - k))) & M32

    def seed(pix, sub, seq=1):
        with np.errstate(over="ignore"):
            pk, rk = sm((U(seq) << U(32)) | pix.astype(U)), sm(sub.astype(U) * U(0xD1B54A32D192ED03))
        a, b = (pk ^ rk) & M32, ((pk >> U(32)) ^ (rk >> U(32))) & M32
        t = a * (b | U(1))
        return (t & M32) ^ b, ((t >> U(32)) ^ a) | U(0x80000000)

    def step(s0, s1):
        t = s1 ^ s0
        return rotl(s0, 26) ^ t ^ ((t << U(9)) & M32), rotl(t, 13)
    s0, s1 = seed(np.array([77]), np.array([9]))
    s0, s1 = step(s0, s1)
    assert (int(s0[0]), int(s1[0])) == _vsl_stream(77, 1, 9, 1)[0]
    from scipy import stats
    uni = lambda w: ((w >> U(8)).astype(np.float64) + 1.0) / 16777216.0

    def chi1(u, bins=1024):
        h = np.bincount((u * bins).astype(np.int64).clip(0, bins - 1), minlength=bins)
        e = u.size / bins
        return stats.chi2.sf(((h - e) ** 2 / e).sum(), bins - 1)

    def chi2(u, v, bins=64):
        h = np.bincount((u * bins).astype(np.int64).clip(0, bins - 1) * bins + (v * bins).astype(np.int64).clip(0, bins - 1), minlength=bins * bins)
        e = u.size / (bins * bins)
        return stats.chi2.sf(((h - e) ** 2 / e).sum(), bins * bins - 1)
    ps = []
    s0, s1 = seed(np.arange(512)[:, None], np.arange(1, 513)[None, :])      # 512 pixels x 512 records
    s0, s1 = np.ascontiguousarray(np.broadcast_to(s0, (512, 512))), np.ascontiguousarray(np.broadcast_to(s1, (512, 512)))
    prev = None
    for _ in range(8):
        s0, s1 = step(s0, s1)
        a, b = uni(s0), uni(s1)
        c = ((((s0 & U(0xFF)) << U(8)) | (s1 & U(0xFF))).astype(np.float64) + 0.5) / 65536.0
        ps += [chi1(a.ravel()), chi1(b.ravel()), chi1(c.ravel()), chi2(a.ravel(), b.ravel()), chi2(a.ravel(), c.ravel()), chi2(b.ravel(), c.ravel()),
               chi2(a[:, :-1].ravel(), a[:, 1:].ravel()), chi2(b[:, :-1].ravel(), b[:, 1:].ravel()),        # neighbouring records
               chi2(a[:-1].ravel(), a[1:].ravel()), chi2(b[:-1].ravel(), b[1:].ravel())]                    # neighbouring pixels
        if prev is not None:                                                                                # consecutive samples of a stream
            ps += [chi2(prev[0].ravel(), a.ravel()), chi2(prev[1].ravel(), b.ravel()), chi2(prev[0].ravel(), b.ravel()), chi2(prev[1].ravel(), a.ravel())]
        prev = (a, b)
    ps = np.array(ps)
    # 108 tests: the smallest p-value of as many uniform ones is below 1e-4 once in a hundred runs; the inputs are fixed, so this is a known
    # answer (tools-side, the same battery on sixteen times the data over five seeds: smallest of 540 p-values 7e-4)
    assert ps.min() > 1e-4 and ps.max() < 1.0 - 1e-4, (ps.min(), ps.max())


def test_vsl_rng_three_way_dependence_is_confined_to_the_low_bits(oracle):
    """ADVICE (round 5): the estimators read the RAW xoroshiro64 state -- no * / ** scrambler -- so consecutive samples are linear images of each
    other: s1' = rotl(s0 ^ s1, 13) exactly.  In terms of the 24-bit uniforms (ua, ub) = (s0 >> 8, s1 >> 8): the top 11 bits of the NEXT ub
    are the LOW 11 bits of ua XOR ub -- a three-way relation no pairwise test sees.  This test states it as a known answer, and then shows
    what the estimators need: at the resolution an integrand can see (the top bits), triples of consecutive draws are jointly uniform
    (three-dimensional chi-square, 32^3 cells), and smooth functions of (ua_n, ub_n, ub_n+1) / (ua_n, ub_n, ua_n+1) average to the
    product of their means within four standard errors.  The low bits of a uniform place a sample within 2^-13 of where its high bits put
    it; what they decide downstream is the NEXT sample's position, as a hash of bits the current sample's geometry does not depend on."""
    from scipy import stats
    U = np.uint64
    M32 = U(0xFFFFFFFF)

    def sm(x):
        with np.errstate(over="ignore"):
            x = x + U(0x9E3779B97F4A7C15)
            x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
            return x ^ (x >> U(31))
    rotl = lambda x, k: ((x << U(k)) | (x >> U(32 - k))) & M32

    def seed(pix, sub, seq=1):
        with np.errstate(over="ignore"):
            pk, rk = sm((U(seq) << U(32)) | pix.astype(U)), sm(sub.astype(U) * U(0xD1B54A32D192ED03))
        a, b = (pk ^ rk) & M32, ((pk >> U(32)) ^ (rk >> U(32))) & M32
        t = a * (b | U(1))
        return (t & M32) ^ b, ((t >> U(32)) ^ a) | U(0x80000000)

    def step(s0, s1):
        t = s1 ^ s0
        return rotl(s0, 26) ^ t ^ ((t << U(9)) & M32), rotl(t, 13)
    s0, s1 = seed(np.arange(768)[:, None], np.arange(1, 769)[None, :])
    s0, s1 = np.ascontiguousarray(np.broadcast_to(s0, (768, 768))).ravel(), np.ascontiguousarray(np.broadcast_to(s1, (768, 768))).ravel()
    assert (int(s0[5 * 768 + 8]), int(s1[5 * 768 + 8])) != (0, 0)
    # the vectorised restatement is the oracle's generator
    r = oa.Rng(); oracle.evo_vsl_rng_init(C.byref(r), 5, 1, 9); oracle.evo_vsl_rng_step(C.byref(r))
    t0, t1 = step(s0[5 * 768 + 8:5 * 768 + 9], s1[5 * 768 + 8:5 * 768 + 9])
    assert (r.s0, r.s1) == (int(t0[0]), int(t1[0]))
    ps, zs = [], []
    uni = lambda w: ((w >> U(8)).astype(np.float64) + 1.0) / 16777216.0
    s0, s1 = step(s0, s1)
    for _ in range(6):
        n0, n1 = step(s0, s1)
        ia, ib, ib2 = s0 >> U(8), s1 >> U(8), n1 >> U(8)
        # the known answer: top 11 bits of the next ub = low 11 bits of (ua ^ ub)
        assert np.array_equal(ib2 >> U(13), (ia ^ ib) & U(0x7FF))
        a, b, a2, b2 = uni(s0), uni(s1), uni(n0), uni(n1)
        for x, y, z in ((a, b, b2), (a, b, a2), (b, a2, b2)):
            cell = ((x * 32).astype(np.int64).clip(0, 31) * 32 + (y * 32).astype(np.int64).clip(0, 31)) * 32 + (z * 32).astype(np.int64).clip(0, 31)
            h = np.bincount(cell, minlength=32 ** 3)
            e = x.size / 32 ** 3
            ps.append(stats.chi2.sf(((h - e) ** 2 / e).sum(), 32 ** 3 - 1))
            # smooth three-way statistics: E[f(x) g(y) h(z)] against E f E g E h (independent uniforms: cos(2 pi k u) has mean 0, variance 1/2)
            for kx, ky, kz in ((1, 1, 1), (1, 2, 3), (3, 1, 2), (5, 7, 11)):
                v = np.cos(2 * np.pi * kx * x) * np.cos(2 * np.pi * ky * y) * np.cos(2 * np.pi * kz * z)
                zs.append(v.mean() / (np.sqrt(0.125) / np.sqrt(v.size)))
            v = (x - 0.5) * (y - 0.5) * (z - 0.5)
            zs.append(v.mean() / ((1.0 / 12.0) ** 1.5 / np.sqrt(v.size)))
        s0, s1 = n0, n1
    ps, zs = np.array(ps), np.array(zs)
    assert ps.min() > 1e-4 and ps.max() < 1.0 - 1e-4, (ps.min(), ps.max())          # 18 three-dimensional tests on fixed inputs: a known answer
    assert np.abs(zs).max() < 4.5, np.abs(zs).max()                                 # 90 z-scores


def test_bvh_matches_brute_force(room_scene, oracle):
    room, s = room_scene
    rng = np.random.RandomState(4)
    for _ in range(3000):
        o = (rng.rand(3) * [10, 8, 5]).astype(np.float32); e = (rng.rand(3) * [10, 8, 5]).astype(np.float32)
        d = (e - o).astype(np.float32)
        assert oracle.evo_occluded(s.h, oa.ptr(o), oa.ptr(d), 1e-4, 1 - 1e-4) == oracle.evo_occluded_brute(s.h, oa.ptr(o), oa.ptr(d), 1e-4, 1 - 1e-4)
    # closest hit: nearest over all triangles, checked by an independent loop over evo_tri_test
    verts = s.verts
    t, b, g = (C.c_float() for _ in range(3))
    for _ in range(200):
        o = (np.array([1, 1, 1]) + rng.rand(3) * [8, 6, 3]).astype(np.float32); d = rng.randn(3).astype(np.float32)
        tri = oracle.evo_closest(s.h, oa.ptr(o), oa.ptr(d), 1e-4, 3e38, 0, C.byref(t), C.byref(b), C.byref(g))
        best, bt = -1, 3e38
        tt, bb, gg = (C.c_float() for _ in range(3))
        for k in range(verts.shape[0]):
            v = verts[k]
            if oracle.evo_tri_test(oa.ptr(v[0:3]), oa.ptr(v[3:6]), oa.ptr(v[6:9]), oa.ptr(o), oa.ptr(d), 1e-4, 3e38, C.byref(tt), C.byref(bb), C.byref(gg)):
                if tt.value < bt:
                    best, bt = k, tt.value
        assert tri == best and (tri < 0 or t.value == bt)


def test_brdf_identities(oracle):
    rng = np.random.RandomState(5)
    for _ in range(200):
        n = rng.randn(3); n /= np.linalg.norm(n); n = n.astype(np.float32)
        w = rng.randn(3); w /= np.linalg.norm(w); w = w.astype(np.float32)
        e = float(rng.rand() * 40)
        mirror = (2 * n * float(n @ w) - w).astype(np.float32)
        # PhongEvalF at the mirror direction = (e+2)/(2 pi)   (rtmaterial.cuh:112-118)
        val = oracle.evo_phong_eval_f(oa.ptr(mirror), oa.ptr(w), oa.ptr(n), e)
        if float(mirror @ (2 * n * float(n @ w) - w)) > 1e-6:
            assert abs(val - (e + 2) / (2 * math.pi)) < 1e-3 * (e + 2)
    # LambertPdfA = GeometryTerm / pi  (rtmaterial.cuh:30-54)
    n1 = np.array([0, 0, 1], np.float32); n2 = np.array([0, 0, -1], np.float32); v = np.array([0.3, 0.2, 2.0], np.float32)
    c1, c2, d2 = float(n1 @ v), float(-(n2 @ v)), float(v @ v)
    assert abs(oracle.evo_lambert_pdf_a(oa.ptr(n1), oa.ptr(n2), oa.ptr(v)) - c1 * c2 / d2 / d2 / math.pi) < 1e-7
    # thresholds: PhongPdfW is 0 for rho_s.x <= 1e-6 (rtmaterial.cuh:83)
    z = np.array([0, 0, 0], np.float32)
    assert oracle.evo_phong_pdf_w(oa.ptr(n1), oa.ptr(v), oa.ptr(v), oa.ptr(z), 10.0) == 0.0


def test_light_tracing_structure_and_energy(room_scene):
    room, s = room_scene
    N, P = 2000, 4
    rec = s.trace_light_paths(1, N, P).reshape(N, P)
    area = s.lib.evo_scene_light_area(s.h)
    # record 0: on-light VPL with flux = I * pi * A (rtlightsource.cuh:71-79, lighttracing.cu:215-225)
    assert (rec["flags"][:, 0] == 1).all()
    want = np.float32(np.array(room.light_intensity[:3], np.float32) * np.float32(math.pi)) * np.float32(area)
    assert np.allclose(rec["flux"][:, 0], want[None, :], rtol=1e-6)
    assert np.allclose(rec["pos"][:, 0, 2], 4.9)                           # all samples on the light quads
    assert (rec["normal"][:, 0, 2] < -0.999).all()
    # flags: inner vertices VPL|photon (+lobe bit), last slot photon only; flux never grows without bound
    inner = rec["flags"][:, 1:P - 1]
    assert set(np.unique(inner & 3).tolist()) <= {0, 3}
    assert set(np.unique(rec["flags"][:, P - 1] & 3).tolist()) <= {0, 2}
    used = rec["flags"] != 0
    assert np.isfinite(rec["flux"][used]).all() and rec["flux"][used].max() < 100 * want.max()
    # a different seed gives a different set; the same seed the same set
    assert rec.tobytes() == s.trace_light_paths(1, N, P).tobytes()
    assert rec.tobytes() != s.trace_light_paths(2, N, P).tobytes()


def test_gather_and_path_tracer_agree_in_expectation(room_scene):
    """Instant radiosity (many VPLs, misMode one) and the NEE path tracer estimate the same image
    (direct + <= 3 indirect bounces): a coarse statistical cross-check of two restated algorithms."""
    room, s = room_scene
    W, H = 24, 16
    room.aspect = W / H
    g = s.primary(W, H)
    fp = dict(camera_pos=room.cam_origin, mis_mode=4, clamping_value=1e9, num_light_paths=400, num_vpl_light_paths=400, photons_per_path=4, do_accumulate=1)
    acc = np.zeros((H, W, 4), np.float32)
    for it in range(3):
        rec = s.trace_light_paths(it, 400, 4)
        s.gather(oa.frame_params(rng_seed=it, **fp), W, H, g, rec, out=acc)
    ir = acc[..., :3] / 3
    pt = np.zeros((H, W, 4), np.float32)
    n_it = 96
    for it in range(n_it):
        s.path_trace(room.cam_origin, it, 3, W, H, g, out=pt)
    pt = pt[..., :3] / n_it
    a, b = ir.mean(axis=(0, 1)), pt.mean(axis=(0, 1))
    assert np.all(np.abs(a - b) < 0.12 * b), (a, b)


def test_progressive_schedule_closed_form(oracle, evplp):
    r0, alpha, cs = 0.05, 0.7, 0.02
    r, c, p, vr, vi = (C.c_float(x) for x in (r0, cs, 0.0, 0.1, 0.0))
    pr, pc, pp = r0, cs, 0.0
    for i in range(1, 101):
        oracle.evo_progressive_step(i, alpha, cs, 30, 300000, C.byref(r), C.byref(c), C.byref(p), 1, C.byref(vr), C.byref(vi))
        pr, pc, pp, _, _ = evplp.progressive_step(i, alpha, cs, 30, 300000, pr, pc, pp)
        assert (r.value, c.value, p.value) == (pr, pc, pp)              # product host code == oracle, bit for bit
    # Knaus-Zwicker: r_n^2 = r_0^2 * prod (i + alpha) / (i + 1)
    want = r0 * math.sqrt(np.prod([(i + alpha) / (i + 1) for i in range(1, 101)]))
    assert abs(r.value - want) < 1e-5 * want
    assert abs(c.value - cs * 100 ** alpha) < 1e-5 * c.value
    assert abs(p.value - (30 / 300000) / math.pi / r.value ** 2) < 1e-4 * p.value
    assert vr.value >= 0.008                                              # floor rtcomphoton.h:1050-1054


def test_photon_fragment_modes_are_complements(oracle):
    """VPL-side weight + photon-side weight = 1 for the MIS modes: checked on the weights the
    restated shader and vplSplat apply to one fixed geometry."""
    ph = np.zeros(2, oa.RECORD_DTYPE)
    ph[0]["pos"] = (0, 0, 2); ph[0]["normal"] = (0, 0, -1); ph[0]["flux"] = (1, 1, 1); ph[0]["flux_dir"] = (0, 0, -1)
    ph[0]["rho_s"] = (1, 1, 1); ph[0]["flags"] = 1
    ph[1]["pos"] = (0.2, 0.1, 0); ph[1]["normal"] = (0, 0, 1); ph[1]["flux"] = (0.7, 0.6, 0.5); ph[1]["flux_dir"] = (-0.1, -0.05, 1)
    ph[1]["rho_d"] = (0.5, 0.5, 0.5); ph[1]["p_select_lambert"] = 1.0; ph[1]["flags"] = 3
    X = np.array([0.21, 0.11, 0.0], np.float32); N = np.array([0, 0, 1], np.float32)
    dif = np.array([0.6, 0.6, 0.6], np.float32); phg = np.array([0, 0, 0, 0], np.float32)
    out0 = np.zeros(3, np.float32); out1 = np.zeros(3, np.float32)
    base = dict(camera_pos=(0, -3, 1), photon_radius=0.05, num_light_paths=10, num_vpl_light_paths=10, photons_per_path=2)
    fp0 = oa.frame_params(mis_mode=0, **base)
    assert oracle.evo_photon_frag(C.byref(fp0), oa.ptr(ph[1:2]), oa.ptr(ph[0:1]), oa.ptr(X), oa.ptr(N), oa.ptr(dif), oa.ptr(phg), oa.ptr(out0)) == 1
    fp1 = oa.frame_params(mis_mode=1, pdf_mc=0.37, **base)
    oracle.evo_photon_frag(C.byref(fp1), oa.ptr(ph[1:2]), oa.ptr(ph[0:1]), oa.ptr(X), oa.ptr(N), oa.ptr(dif), oa.ptr(phg), oa.ptr(out1))
    w_photon = out1 / out0
    assert np.allclose(w_photon, w_photon[0]) and 0 < w_photon[0] < 1
    far = np.array([5, 5, 0], np.float32)
    assert oracle.evo_photon_frag(C.byref(fp0), oa.ptr(ph[1:2]), oa.ptr(ph[0:1]), oa.ptr(far), oa.ptr(N), oa.ptr(dif), oa.ptr(phg), oa.ptr(out0)) == 0   # outside the kernel radius: discard


def test_vpl_splat_known_answers(oracle):
    """vplSplat (rt/lighttracing.cu:275-346) on a geometry whose result can be written down by hand: shading point at
    the origin facing +z, VPL two units above it facing down, both Lambertian with rho = 0.5, unit flux.
      v12 = (0,0,2), cos1 = cos2 = 2 (un-normalised, :284-287), d^2 = 4, G = cos1 cos2 / d^4 = 1/4 (:303)
      brdf1 = brdf2 = 0.5 / pi;  one: flux brdf1 brdf2 G (:309-312);  geometryClamp: G -> min(G, c) (:333-336);
      geometryBrdfClamp: min(brdf1 G brdf2, c) (:338-344);  MIS modes: pdf_de = LambertPdfA p_sel = G / pi (:318-320),
      weight = pdfMc/(pdfMc+pdf_de), [pdfMc > pdf_de], pdfMc^2/(pdfMc^2+pdf_de^2) (:321-331)."""
    rec = np.zeros(1, oa.RECORD_DTYPE)
    rec[0]["pos"] = (0, 0, 2); rec[0]["normal"] = (0, 0, -1); rec[0]["flux"] = (1, 1, 1); rec[0]["flux_dir"] = (0, 0, 1)
    rec[0]["rho_d"] = (0.5, 0.5, 0.5); rec[0]["p_select_lambert"] = 1.0; rec[0]["flags"] = 1
    wi10 = np.array([0, 0.6, 0.8], np.float32); p1 = np.zeros(3, np.float32); n1 = np.array([0, 0, 1], np.float32)
    rd = np.full(3, 0.5, np.float32); rs = np.zeros(3, np.float32)
    G = 0.25; f = 0.5 / math.pi; plain = f * f * G
    pdf_mc = 0.1; pdf_de = G / math.pi
    want = {0: plain, 1: plain * pdf_mc / (pdf_mc + pdf_de), 2: plain * (1.0 if pdf_mc > pdf_de else 0.0), 3: plain * pdf_mc ** 2 / (pdf_mc ** 2 + pdf_de ** 2),
            4: f * f * min(G, 0.1), 5: min(plain, 0.004)}
    for mode, w in want.items():
        fp = oa.frame_params(camera_pos=(0, 3, 4), mis_mode=mode, pdf_mc=pdf_mc, clamping_value=0.1 if mode == 4 else 0.004,
                             num_light_paths=1, num_vpl_light_paths=1, photons_per_path=1)
        out = np.zeros(3, np.float32)
        oracle.evo_vpl_splat_pair(C.byref(fp), oa.ptr(wi10), oa.ptr(p1), oa.ptr(n1), oa.ptr(rd), oa.ptr(rs), 0.0, oa.ptr(rec), 1, oa.ptr(out))
        assert np.allclose(out, w, rtol=2e-6, atol=0), (mode, out, w)
        oracle.evo_vpl_splat_pair(C.byref(fp), oa.ptr(wi10), oa.ptr(p1), oa.ptr(n1), oa.ptr(rd), oa.ptr(rs), 0.0, oa.ptr(rec), 0, oa.ptr(out))
        assert (out == 0).all()                                  # occluded: no contribution (:296-298)
    # back-facing VPL: cos2 <= 0 -> culled before the shadow ray (:288)
    rec[0]["normal"] = (0, 0, 1)
    fp = oa.frame_params(camera_pos=(0, 3, 4), mis_mode=0, num_light_paths=1, num_vpl_light_paths=1, photons_per_path=1)
    out = np.ones(3, np.float32)
    oracle.evo_vpl_splat_pair(C.byref(fp), oa.ptr(wi10), oa.ptr(p1), oa.ptr(n1), oa.ptr(rd), oa.ptr(rs), 0.0, oa.ptr(rec), 1, oa.ptr(out))
    assert (out == 0).all()
    # a Phong receiver seen along its mirror direction: brdf1 += rho_s (e + 2) / (2 pi) (rtmaterial.cuh:112-118)
    rec[0]["normal"] = (0, 0, -1)
    rs2 = np.full(3, 0.2, np.float32); e = 10.0
    up = np.array([0, 0, 1], np.float32)
    oracle.evo_vpl_splat_pair(C.byref(fp), oa.ptr(up), oa.ptr(p1), oa.ptr(n1), oa.ptr(rd), oa.ptr(rs2), e, oa.ptr(rec), 1, oa.ptr(out))
    assert np.allclose(out, (f + 0.2 * (e + 2) / (2 * math.pi)) * f * G, rtol=2e-6)


def test_photon_fragment_known_answers(oracle):
    """photonsplatinstanced.frag:146-240 on a hand-computable geometry: photon at the origin on a +z surface, its
    predecessor two units above facing down (Lambertian, p_select = 1), shading point 0.01 away inside r = 0.05.
      brdf1 = rho_d / pi (frag:42-50);  k = 1 / (pi r^2) / N (frag:196);  w12 = (0,0,1), d^2 = 4
      mixPdfW = cos / pi * p_sel = 1/pi (frag:65-69,184-187);  mixPdfA = mixPdfW * (n1.w12) / d^2 = 1/(4 pi) (frag:189)
      one: brdf1 k flux;  balance / max / power2: * heuristic(mixPdfA, pdfMc) (frag:199-213)
      geometryClamp: * max(G - c, 0) / G with G = 1/4 (frag:214-222);  geometryBrdfClamp: k flux max(brdf1 brdf2 G - c, 0) / (G brdf2)"""
    ph = np.zeros(1, oa.RECORD_DTYPE); prev = np.zeros(1, oa.RECORD_DTYPE)
    prev[0]["pos"] = (0, 0, 2); prev[0]["normal"] = (0, 0, -1); prev[0]["flux_dir"] = (0, 0, -1); prev[0]["rho_d"] = (0.5, 0.5, 0.5)
    prev[0]["p_select_lambert"] = 1.0; prev[0]["flags"] = 1
    ph[0]["pos"] = (0, 0, 0); ph[0]["normal"] = (0, 0, 1); ph[0]["flux"] = (0.7, 0.6, 0.5); ph[0]["flux_dir"] = (0, 0, 1)
    ph[0]["rho_d"] = (0.4, 0.4, 0.4); ph[0]["p_select_lambert"] = 1.0; ph[0]["flags"] = 3
    X = np.array([0.01, 0, 0], np.float32); N = np.array([0, 0, 1], np.float32)
    dif = np.full(3, 0.6, np.float32); phg = np.zeros(4, np.float32)
    r, npaths, pdf_mc = 0.05, 10, 0.05
    flux = np.array([0.7, 0.6, 0.5])
    brdf1 = 0.6 / math.pi; brdf2 = 0.5 / math.pi; k = 1.0 / (math.pi * r * r) / npaths
    mix_a = 1.0 / (4.0 * math.pi); G = 0.25
    base = brdf1 * k * flux
    want = {0: base, 1: base * mix_a / (mix_a + pdf_mc), 2: base * (1.0 if mix_a > pdf_mc else 0.0), 3: base * mix_a ** 2 / (mix_a ** 2 + pdf_mc ** 2),
            4: base * max(G - 0.1, 0.0) / G, 5: k * flux * max(brdf1 * brdf2 * G - 0.004, 0.0) / (G * brdf2)}
    for mode, w in want.items():
        fp = oa.frame_params(camera_pos=(0, -3, 4), mis_mode=mode, pdf_mc=pdf_mc, clamping_value=0.1 if mode == 4 else 0.004, photon_radius=r,
                             num_light_paths=npaths, num_vpl_light_paths=npaths, photons_per_path=2)
        out = np.zeros(3, np.float32)
        assert oracle.evo_photon_frag(C.byref(fp), oa.ptr(ph), oa.ptr(prev), oa.ptr(X), oa.ptr(N), oa.ptr(dif), oa.ptr(phg), oa.ptr(out)) == 1
        assert np.allclose(out, w, rtol=3e-6, atol=0), (mode, out, w)
    # VPL weight + photon weight = 1 for the three MIS heuristics with the same pdfs (the energy-compensation identity)
    for mode, wp in ((1, mix_a / (mix_a + pdf_mc)), (3, mix_a ** 2 / (mix_a ** 2 + pdf_mc ** 2))):
        wv = {1: pdf_mc / (pdf_mc + mix_a), 3: pdf_mc ** 2 / (pdf_mc ** 2 + mix_a ** 2)}[mode]
        assert abs(wp + wv - 1.0) < 1e-12


def test_shared_direction_sampling_math_against_libm(oracle):
    """evplp_amd/csrc/ev_math.h (one sin / cos / pow for the oracle AND the kernels, so that light-path records compare bit for
    bit) is an independent implementation: check it against double-precision libm over the ranges the samplers use."""
    import ctypes as C
    rng = np.random.RandomState(5)
    s, c = C.c_float(), C.c_float()
    xs = np.concatenate([rng.rand(20000).astype(np.float32) * np.float32(6.2831855), np.linspace(0, 6.2831855, 5001, dtype=np.float32)])
    worst = 0.0
    for x in xs:
        oracle.evo_math_sincos(float(x), C.byref(s), C.byref(c))
        for got, ref in ((s.value, math.sin(float(x))), (c.value, math.cos(float(x)))):
            worst = max(worst, abs(got - ref) / max(float(np.spacing(np.float32(abs(ref)))), 2.0 ** -30))
    assert worst <= 2.0, worst                       # ulps of the result (absolute 2^-30 floor at the zero crossings)
    worst = 0.0
    for _ in range(20000):
        x = float(np.float32(rng.rand())); y = float(np.float32(rng.choice([rng.rand(), 1.0 / (1.0 + rng.rand() * 100.0), rng.rand() * 200.0])))
        if x <= 0.0:
            continue
        got, ref = oracle.evo_math_pow(x, y), x ** y
        if ref > 1e-37:
            worst = max(worst, abs(got - ref) / float(np.spacing(np.float32(ref))))
    assert worst <= 0.51, worst
    assert oracle.evo_math_pow(0.0, 2.0) == 0.0 and oracle.evo_math_pow(0.3, 0.0) == 1.0 and oracle.evo_math_pow(1.0, 77.0) == 1.0
    assert oracle.evo_math_pow(0.25, 0.5) == 0.5


# ---------------------------------------------------------------------------------------------------------------------
# Vouching for the oracle's VSL estimators (vslSplat, rt/lighttracing.cu:395-686) -- the most intricate function on the path.
# The reference cannot be run here, so the restatement is checked against (a) the limit it must have,
# (b) the integral every one of its three estimators -- and their MIS combination -- must converge to, computed by quadrature,
# (c) a single-sample answer derived by hand from a known RNG draw.

def _vsl_setup(glossy=True):
    n = lambda v: (np.array(v, np.float64) / np.linalg.norm(v)).astype(np.float32)
    rec = np.zeros(1, oa.RECORD_DTYPE)
    rec[0]["pos"] = (0.4, 0.3, 1.5); rec[0]["normal"] = n((-0.2, -0.1, -1.0)); rec[0]["flux"] = (1.0, 0.8, 0.6)
    rec[0]["flux_dir"] = n((0.1, -0.3, -0.9)); rec[0]["rho_d"] = (0.4, 0.4, 0.4)
    rec[0]["rho_s"] = (0.2, 0.2, 0.2) if glossy else (0, 0, 0); rec[0]["phong_exp"] = 5.0 if glossy else 0.0
    rec[0]["p_select_lambert"] = 0.4 / 0.6 if glossy else 1.0; rec[0]["flags"] = 1
    px = dict(wi10=n((0.3, -0.2, 0.9)), p1=np.zeros(3, np.float32), n1=np.array([0, 0, 1], np.float32),
              rd=np.full(3, 0.5, np.float32), rs=np.full(3, 0.3 if glossy else 0.0, np.float32), e=8.0 if glossy else 0.0)
    return rec, px


def _vsl_pair(oracle, rec, px, radius, only, samples, stream=(5, 7, 11), visible=1):
    fp = oa.frame_params(camera_pos=(0, 0, 0), vsl_radius=radius, vsl_inv_pi_radius2=1.0 / (math.pi * radius * radius),
                         num_light_paths=1, num_vpl_light_paths=1, photons_per_path=1)
    out = np.zeros(3, np.float32)
    oracle.evo_vsl_splat_pair(C.byref(fp), oa.ptr(px["wi10"]), oa.ptr(px["p1"]), oa.ptr(px["n1"]), oa.ptr(px["rd"]), oa.ptr(px["rs"]), px["e"],
                              oa.ptr(rec), visible, stream[0], stream[1], stream[2], only, samples, oa.ptr(out))
    return out.astype(np.float64)


def _vsl_integral_by_quadrature(rec, px, radius, nz=600, nphi=720):
    """flux / (pi r^2) * integral over the cone (axis = direction to the VSL, half angle asin(r / d)) of
    cos1 cos2 brdf1 brdf2 d_omega  -- the quantity vslSampleCone / vslSampleBrdf1 / vslSampleBrdf2 each estimate (:395-594)."""
    f64 = lambda a: np.asarray(a, np.float64)
    p2, n2, fdir = f64(rec[0]["pos"]), f64(rec[0]["normal"]), f64(rec[0]["flux_dir"])
    n1, wi10 = f64(px["n1"]), f64(px["wi10"])
    v12 = p2 - f64(px["p1"]); d = np.linalg.norm(v12); axis = v12 / d
    cos_max = math.cos(math.asin(min(radius / d, 1.0)))
    t = np.cross(axis, [1.0, 0, 0]); t /= np.linalg.norm(t); b = np.cross(axis, t)
    z = 1.0 - (np.arange(nz) + 0.5) / nz * (1.0 - cos_max); phi = (np.arange(nphi) + 0.5) / nphi * 2 * math.pi
    Z, PH = np.meshgrid(z, phi, indexing="ij"); S = np.sqrt(np.maximum(1 - Z * Z, 0))
    w = Z[..., None] * axis + (S * np.cos(PH))[..., None] * t + (S * np.sin(PH))[..., None] * b
    c1 = np.maximum(w @ n1, 0); c2 = np.maximum(-(w @ n2), 0)
    def phong(out, inn, nrm, e):                                  # PhongEvalF, rtmaterial.cuh:112-118
        r = -inn + 2.0 * nrm * (inn @ nrm)[..., None] if inn.ndim > 1 else -inn + 2.0 * nrm * float(inn @ nrm)
        dd = np.maximum(np.sum(out * r, axis=-1), 0)
        return np.where(dd <= 1e-6, 0.0, (e + 2) * np.power(np.maximum(dd, 1e-300), e) / (2 * math.pi))
    ph1 = phong(np.broadcast_to(wi10, w.shape), w, n1, px["e"])
    ph2 = phong(-w, np.broadcast_to(fdir, w.shape), n2, float(rec[0]["phong_exp"]))
    dom = (1.0 - cos_max) / nz * (2 * math.pi / nphi)
    out = []
    for ch in range(3):
        f1 = float(px["rd"][ch]) / math.pi + float(px["rs"][ch]) * ph1
        f2 = float(rec[0]["rho_d"][ch]) / math.pi + float(rec[0]["rho_s"][ch]) * ph2
        out.append(float(rec[0]["flux"][ch]) / (math.pi * radius * radius) * float(np.sum(c1 * c2 * f1 * f2)) * dom)
    return np.array(out)


@pytest.mark.parametrize("glossy", [False, True])
def test_vsl_estimators_each_converge_to_the_cone_integral(oracle, glossy):
    """(b) the cone estimator alone, the pixel-BRDF estimator alone, the VSL-BRDF estimator alone (MIS weight forced to 1 by the
    test hook) and the reference's MIS combination all estimate flux / (pi r^2) * int_cone cos1 cos2 f1 f2: each is compared
    with a 600 x 720-point quadrature of that integral."""
    rec, px = _vsl_setup(glossy)
    radius = 0.9                                         # r / d = 0.57: a wide cone, so the BRDF estimators land in it often
    want = _vsl_integral_by_quadrature(rec, px, radius)
    assert (want > 0).all()
    n = 300000
    for only, tol in ((1, 0.01), (2, 0.03), (3, 0.03), (0, 0.01)):
        got = np.mean([_vsl_pair(oracle, rec, px, radius, only, n, stream=(3, 1, k)) for k in range(4)], axis=0)
        assert np.all(np.abs(got - want) <= tol * want), (only, got, want)


def test_vsl_small_radius_limit_is_the_vpl(oracle, room_scene):
    """(a) r -> 0: the cone shrinks onto the connection, the integrand is constant over it and
    flux / (pi r^2) * cos1 cos2 f1 f2 * Omega  ->  flux f1 f2 cos1 cos2 / d^2 = vplSplat with misMode one (:309-312)."""
    # (fp32 note: Omega = 2 pi (1 - cos t) cancels catastrophically for r / d below ~1e-3 -- the reference floors the radius at 0.008,
    # rtcomphoton.h:1050-1054 -- so the limit is taken at r / d = 0.02 and the first-order variation of the integrand over the cone
    # is averaged out with many samples: what is left is O((r/d)^2))
    for glossy, tol in ((False, 2e-3), (True, 1e-2)):
        rec, px = _vsl_setup(glossy)
        fp = oa.frame_params(camera_pos=(0, 0, 0), mis_mode=0, num_light_paths=1, num_vpl_light_paths=1, photons_per_path=1)
        vpl = np.zeros(3, np.float32)
        oracle.evo_vpl_splat_pair(C.byref(fp), oa.ptr(px["wi10"]), oa.ptr(px["p1"]), oa.ptr(px["n1"]), oa.ptr(px["rd"]), oa.ptr(px["rs"]), px["e"], oa.ptr(rec), 1, oa.ptr(vpl))
        d = float(np.linalg.norm(rec[0]["pos"]))
        vsl = _vsl_pair(oracle, rec, px, 0.02 * d, 0, 40000)
        assert (vpl > 0).all() and np.all(np.abs(vsl - vpl) <= tol * vpl), (glossy, vsl, vpl)
        assert (_vsl_pair(oracle, rec, px, 0.02 * d, 0, 0, visible=0) == 0).all()      # occluded centre ray: nothing (:612-616)
    # ... and as whole gathers over a room (visibility, record loop, normalisation included)
    room, s = room_scene
    W, H = 24, 16
    room.aspect = W / H
    g = s.primary(W, H)
    rec = s.trace_light_paths(3, 64, 4)
    kw = dict(camera_pos=room.cam_origin, num_light_paths=64, num_vpl_light_paths=64, photons_per_path=4, rng_seed=2)
    r = 0.02
    vsl, pairs_v = s.gather(oa.frame_params(vsl_radius=r, vsl_inv_pi_radius2=1.0 / (math.pi * r * r), **kw), W, H, g, rec, vsl=True)
    vpl, pairs_p = s.gather(oa.frame_params(mis_mode=0, **kw), W, H, g, rec)
    assert pairs_v == pairs_p and vpl[..., :3].max() > 0
    a, b = vsl[..., :3].astype(np.float64), vpl[..., :3].astype(np.float64)
    assert np.linalg.norm(a - b) <= 2e-2 * np.linalg.norm(b)


def test_vsl_cone_sample_known_answer(oracle):
    """(c) one cone sample, by hand.  Pixel at the origin facing +z, VSL two units above it facing down, both Lambertian:
    every direction w of the cone has cos1 = cos2 = w.z, so the cone estimator (:395-446) returns
        flux / (pi r^2) * z^2 * (rho1 / pi) (rho2 / pi) * Omega,   Omega = 2 pi (1 - cos t),  cos t = sqrt(1 - (r/d)^2),
        z = 1 - u_b (1 - cos t)   (SquareToSolidAngle, :382-390; the rotation about the cone axis +z keeps z),
    with u_b the second uniform of the stream's first step (the sample's first draw is the unused chooseMaterial of :414, then the
    azimuth, then u_b)."""
    rec = np.zeros(1, oa.RECORD_DTYPE)
    rec[0]["pos"] = (0, 0, 2); rec[0]["normal"] = (0, 0, -1); rec[0]["flux"] = (1.0, 0.5, 0.25); rec[0]["flux_dir"] = (0, 0, -1)
    rec[0]["rho_d"] = (0.4, 0.4, 0.4); rec[0]["p_select_lambert"] = 1.0; rec[0]["flags"] = 1
    px = dict(wi10=np.array([0, 0.6, 0.8], np.float32), p1=np.zeros(3, np.float32), n1=np.array([0, 0, 1], np.float32),
              rd=np.full(3, 0.5, np.float32), rs=np.zeros(3, np.float32), e=0.0)
    radius, d = 0.5, 2.0
    cos_t = math.sqrt(1 - (radius / d) ** 2); omega = 2 * math.pi * (1 - cos_t)
    for stream in ((5, 7, 11), (0, 0, 1), (123, 4, 9)):
        u_b = ((_vsl_stream(*stream, 1)[0][1] >> 8) + 1) / 16777216.0
        z = 1 - u_b * (1 - cos_t)
        want = np.array([1.0, 0.5, 0.25]) / (math.pi * radius ** 2) * z * z * (0.5 / math.pi) * (0.4 / math.pi) * omega
        got = _vsl_pair(oracle, rec, px, radius, 1, 1, stream=stream)
        assert np.allclose(got, want, rtol=2e-5, atol=0), (stream, got, want)
        # the MIS weight of that sample (:433-445): pdfCone / (pdf1 + pdf2 + pdfCone), pdf1 = pdf2 = z (LambertPdfW has no 1/pi in
        # the CUDA source, rtmaterial.cuh:40-44; p_select = 1) -- read off a run whose two BRDF samples cannot land in the cone
    # numSamples (:632) = (int)(halfCone / pi * 2 * 100) + 1
    half = math.asin(radius / d)
    n_ref = int(half / math.pi * 2 * 100) + 1
    a = _vsl_pair(oracle, rec, px, radius, 1, 0, stream=(1, 1, 1)); b = _vsl_pair(oracle, rec, px, radius, 1, n_ref, stream=(1, 1, 1))
    assert (a == b).all() and n_ref == 17


def test_icosphere_proxy_footprint_against_the_ideal_sphere(oracle):
    """The one known semantic deviation of the splat, measured (deviation 4): the reference rasterises an
    inscribed 42-vertex / 80-face icosphere per photon with the depth test on and face culling OFF
    (rtcomphoton.h:632-655, 789-837; photonsplatinstanced.vert:28-33, .geom:16-32); the build tests the sphere itself
    (SURVEY A.4).  Same pixels, same photons, both footprints (oracle/evplp_oracle.c evo_splat_photons_proxy): config-#3-like
    radius (0.003 x bounding-sphere radius, ~4 px at 1024^2) on the box room."""
    room = scenes.box_room(seed=11, n_boxes=6, tess=2, textured=False)
    s = oa.Scene(room)
    W = H = 1024
    rows = (480, 544)
    g = s.primary(W, H, rows=rows)
    oracle.evo_scene_bounding_sphere_radius.restype = C.c_float
    bsr = oracle.evo_scene_bounding_sphere_radius(s.h)
    N, P = 120000, 4
    rec = s.trace_light_paths(0, N, P)
    out = {}
    for frac in (0.003, 0.006):
        fp = oa.frame_params(camera_pos=room.cam_origin, mis_mode=0, photon_radius=frac * bsr, num_light_paths=N, num_vpl_light_paths=N, photons_per_path=P)
        ideal, proxy, st = oa.splat_proxy(fp, s.camera(), W, H, g[:4], rec, rows=rows)
        # the ideal image of evo_splat_photons_proxy IS evo_splat_photons' (same pairs, same fragment values)
        ref, pairs = oa.splat(fp, W, H, g[:4], rec, rows=rows)
        assert pairs == int(st[0])
        assert np.allclose(ideal[..., :3], ref[..., :3], rtol=1e-5, atol=1e-9)
        I = ideal[rows[0]:rows[1], :, :3].astype(np.float64); Q = proxy[rows[0]:rows[1], :, :3].astype(np.float64)
        missed, double, frags = st[1] / st[0], st[2] / st[0], st[3] / st[0]
        ratio = Q.sum() / I.sum()
        out[frac] = (missed, double, frags, ratio)
        print(f"proxy vs ideal, r = {frac} R: {int(st[0])} pairs inside the radius; the proxy misses {100 * missed:.2f} %, counts {100 * double:.2f} % twice "
              f"({frags:.4f} fragments per pair); photon-image energy {100 * (ratio - 1):+.2f} %")
        # an inscribed polyhedron under-covers the silhouette (a few percent of the disc) and, without culling, double counts the
        # surface points that lie behind both of its faces: a few percent either way, a net loss
        assert 0.02 < missed < 0.09 and 0.005 < double < 0.06 and 0.95 < ratio < 1.0
    # the coverage statistics are a property of the shape, not of the radius
    assert abs(out[0.003][2] - out[0.006][2]) < 0.01
