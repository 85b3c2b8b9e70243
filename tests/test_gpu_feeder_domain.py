"""light_trace_kernel and path_trace_pixel against float64, vertex by vertex and pixel by pixel (tests/feeder_domain.py).

The kernels run the cases of test_feeder_domain_host.py -- the patch room with light exponents 0 and 5; 200 light paths (three full wavefronts
and one of eight lanes) of P = 2, 4, 7 slots under two seeds; the path tracer with 1, 2 and 3 bounces on the uploaded 44 x 28 receiver -- and
are held to the same restatement under TWICE the K measured for the fp32 oracle there, the project's rule for the shading domain: the
path-tracer unit is built with contraction allowed, the oracle is not.
    records:  flags, untextured materials and the zeroed tail exactly; |x - f64| <= K 2^-24 kappa scale + 1e-20 for the rest    (K = 2)
    pixels:   |x - f64| <= K 2^-24 sum kappa_term |term| + n_terms 2^-24 sum |term| + 1e-20 on every decided pixel               (K = 4)
There is no allowance for pixels that "took another path": a pixel is decided or it is compared with nothing, and at most 1 % of a case's
pixels (paths) may be undecided.  Light paths are also traced in slices [0, 70), [70, 130), [130, 200) -- starts that are no multiple of 64
-- into a buffer that holds 1e30 in every word, and by all five tree builders.  The path tracer writes over an accumulator that holds 7
everywhere: stencilled-off pixels, the padding lanes of ragged tiles and the rows below H of the padded plane keep it.  One case goes
through evplp_path_trace_batch with two samples, on the G-buffer that call draws for itself.

Measured on an MI355X, 2026-10-21 (`pytest -s -m gpu tests/test_gpu_feeder_domain.py` prints them): light_trace_kernel, error / (2^-24 kappa
scale) at its worst, 0.51 - 0.74 with light exponent 0 and 0.37 - 0.70 with exponent 5 -- the oracle's figures, as bit-identical records must give
-- with 0 - 2 of 200 paths undecided; the slices and the five builders give the whole's bytes.  path_trace, error / bar at its worst, 0.221 for
one sample and 0.176 for two with exponent 0, 0.299 - 0.318 and 0.191 - 0.214 with exponent 5 (K = 4), 1 - 3 and 1 - 6 of 1208 pixels
undecided; path_trace_batch 0.189 with 8 of 1232 undecided.  Every test takes 0.1 - 1.1 s.
"""
import numpy as np
import pytest

import feeder_domain as fd
import oracle_api as oa
from test_feeder_domain_host import K_ORACLE_LT, K_ORACLE_PT, LT_CASES, PT_CASES, check_lt, check_pt

pytestmark = pytest.mark.gpu

K_GPU_LT = 2 * K_ORACLE_LT
K_GPU_PT = 2 * K_ORACLE_PT
W, H = fd.W, fd.H
SLICES = ((0, 70), (70, 130), (130, 200))
BUILDER_CASE = (5.0, 4)


@pytest.fixture(scope="module")
def dom(oracle):
    return fd.Domain(oa)


def big_records(evplp, c):
    n = c.buffer_bytes(evplp.BUF_RECORDS) // 4
    return np.full(n, fd.BIG, np.float32).view(evplp.RECORD_DTYPE)


def trace(evplp, c, seed, slices=None):
    c.upload(evplp.BUF_RECORDS, big_records(evplp, c))
    if slices is None:
        c.trace_light_paths(seed)
    else:
        for b, e in slices:
            c.trace_light_paths(seed, b, e - b)
    return c.download(evplp.BUF_RECORDS)


@pytest.mark.parametrize("e, P", LT_CASES)
def test_light_trace_kernel(evplp, dom, e, P):
    builders = [evplp.BVH_SAH] + ([evplp.BVH_LBVH, evplp.BVH_SBVH, evplp.BVH_LBVH_GPU, evplp.BVH_PLOC_GPU] if (e, P) == BUILDER_CASE else [])
    whole = {}
    for builder in builders:
        with evplp.Context(W, H, fd.LT_PATHS, fd.LT_PATHS, P, bvh_builder=builder, deterministic=True) as c:
            dom.scenes[e].upload(c)
            for seed in fd.LT_SEEDS:
                rec = trace(evplp, c, seed)
                assert rec.shape[0] == fd.LT_PATHS * P
                if builder == evplp.BVH_SAH:
                    r = fd.check_light_paths(dom.geo[e], rec, seed, P)
                    check_lt(r, K_GPU_LT, (e, P, seed))
                    whole[seed] = rec.tobytes()
                    print(f"\nlight_trace_kernel, exponent {e:g}, P = {P}, seed {seed:#x}: worst error / (2^-24 kappa scale) = {r.worst:.2f} (K = {K_GPU_LT}); "
                          f"{r.undecided} undecided of {r.paths} paths; {r.compared} comparisons")
                    assert trace(evplp, c, seed, SLICES).tobytes() == whole[seed], ("the slices do not give the whole's bytes", e, P, seed)
                    # one slice alone leaves every other path's slots as they were
                    part = trace(evplp, c, seed, SLICES[1:2])
                    b, n = SLICES[1][0] * P, SLICES[1][1] * P
                    assert part[b:n].tobytes() == rec[b:n].tobytes()
                    assert np.all(part[:b].view(np.float32) == np.float32(fd.BIG)) and np.all(part[n:].view(np.float32) == np.float32(fd.BIG))
                else:                                   # the hits do not depend on the tree
                    assert rec.tobytes() == whole[seed], ("builder", builder, e, P, seed)


def pt_context(evplp, dom, e, gbuf=True):
    c = evplp.Context(W, H, 32, 32, 2, deterministic=True)
    dom.scenes[e].upload(c)
    if gbuf:
        for b, plane in zip((evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG), dom.gbuf):
            pad = np.zeros((c.local_rows, W, 4), np.float32); pad[:H] = plane
            c.upload(b, pad)
    return c


def check_rays(st, ref, bounces, what):
    """pairs = the stencilled pixels; rays = the restatement's over the decided pixels + the device's own for the undecided, 1 .. 1 + 2 bounces each"""
    n_und = int((~ref.decided & ref.stencil).sum())
    assert st["pairs"] == int(ref.stencil.sum()), (what, st["pairs"])
    rest = st["rays"] - int(ref.rays[ref.decided].sum())
    assert n_und * 1 <= rest <= n_und * (1 + 2 * bounces), (what, st["rays"], rest, n_und)


@pytest.mark.parametrize("e, bounces", PT_CASES)
def test_path_trace(evplp, dom, e, bounces):
    s0, s1 = fd.PT_SEEDS
    ref0, ref1 = dom.pt_ref(e, s0, bounces), dom.pt_ref(e, s1, bounces)
    with pt_context(evplp, dom, e) as c:
        assert c.local_rows > H                      # (28 rows: the padded plane has rows the frame does not)
        # accumulate off, over an accumulator that holds 7 everywhere
        c.upload(evplp.BUF_VPL_ACCUM, np.full((c.local_rows, W, 4), 7.0, np.float32))
        c.path_trace(fd.CAMERA, s0, bounces, accumulate=False)
        plane = c.download(evplp.BUF_VPL_ACCUM)
        got = plane[:H]
        assert np.all(plane[H:] == 7.0), "a padding lane below the frame wrote its texel"
        assert np.all(got[~dom.stencil] == 7.0), "a stencilled-off pixel was written"
        assert np.all(got[dom.stencil][:, 3] == 0.0)
        worst, und = check_pt(got, ref0, K_GPU_PT, ("path_trace", e, bounces))
        check_rays(c.pass_stats(evplp.PASS_PATH_TRACE), ref0, bounces, ("single", e, bounces))
        # accumulate on, twice, from a clear accumulator
        c.clear_accumulators()
        c.path_trace(fd.CAMERA, s0, bounces, accumulate=True)
        c.path_trace(fd.CAMERA, s1, bounces, accumulate=True)
        plane = c.download(evplp.BUF_VPL_ACCUM)
        assert np.all(plane[H:] == 0.0) and np.all(plane[:H][~dom.stencil] == 0.0)
        worst2, und2 = check_pt(plane[:H], fd.add_images(ref0, ref1), K_GPU_PT, ("path_trace accumulated", e, bounces))
        check_rays(c.pass_stats(evplp.PASS_PATH_TRACE), ref1, bounces, ("second sample", e, bounces))
    print(f"\npath_trace, exponent {e:g}, {bounces} bounces: error / bar {worst:.3f} (one sample), {worst2:.3f} (two), K = {K_GPU_PT}; "
          f"undecided {und} and {und2} of {int(dom.stencil.sum())}")


def test_path_trace_batch(evplp, dom):
    """two samples in one call, on the G-buffer the call draws from the scene's own camera (the same jitter twice: one G-buffer)"""
    e, bounces = 5.0, 3
    cam = dom.scenes[e].cam_origin
    with pt_context(evplp, dom, e, gbuf=False) as c:
        c.clear_accumulators()
        c.path_trace_batch(cam, [(0.0, 0.0), (0.0, 0.0)], list(fd.PT_SEEDS), bounces)
        st = c.pass_stats(evplp.PASS_PATH_TRACE)
        gbuf = [c.download(b)[:H] for b in (evplp.BUF_GBUF_POSITION, evplp.BUF_GBUF_NORMAL, evplp.BUF_GBUF_DIFFUSE, evplp.BUF_GBUF_PHONG)]
        plane = c.download(evplp.BUF_VPL_ACCUM)
    refs = [fd.path_image_f64(dom.geo[e], gbuf, None, cam, s, bounces) for s in fd.PT_SEEDS]
    both = fd.add_images(*refs)
    assert int(both.stencil.sum()) > 1000 and np.all(plane[H:] == 0.0) and np.all(plane[:H][~both.stencil] == 0.0)
    worst, und = check_pt(plane[:H], both, K_GPU_PT, "path_trace_batch")
    n_und = [int((~r.decided & r.stencil).sum()) for r in refs]
    assert st["pairs"] == 2 * int(both.stencil.sum())
    rest = st["rays"] - sum(int(r.rays[r.decided].sum()) for r in refs)
    assert sum(n_und) <= rest <= sum(n_und) * (1 + 2 * bounces), (st["rays"], rest, n_und)
    print(f"\npath_trace_batch, exponent {e:g}, {bounces} bounces, two samples: error / bar {worst:.3f} (K = {K_GPU_PT}); undecided {und} of {int(both.stencil.sum())}")
