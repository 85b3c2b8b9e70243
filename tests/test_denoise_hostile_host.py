"""The hostile denoiser cases of tests/denoise_hostile.py are what they claim, and their bars are reachable by the references alone (no GPU).

The composite and the variance come from denoise_hostile.host_inputs(): resolve_kernel's expression and the noise tracker's formula
(test_gpu_noise.numpy_variance) on the case's own accumulator states, in numpy.

Sensitivity bar.  restate() is run a second time with exp, pow and sqrt evaluated in float64 and rounded to fp32: the largest relative
difference between the two restatements (rel_err: |a - b| / max(|b|, 1e-6 max |b|)) is how far those functions' last bits can carry on
that case.  The GPU's bar against restate() is max(1e-4, 8 x that): 1e-4 is the project's own bar for this restatement, and the factor 8
allows the device's expf / powf / sqrtf a few ulp where numpy's are within one.  8 x the figure must stay below 1e-3 or the case cannot
decide anything.  float64 bar.  restate() against statement64() on smooth, holes, dark and bright is the distance between the fp32
operation order and float64; the GPU's bar against statement64() is 4 x that figure.  zero_variance is excluded from that comparison:
with s = 0 the luminance term is |l_p - l_q| / 1e-10, which turns an fp32 rounding of a luminance (1e-8 after the first pass's quotient)
into a weight of e^-100 or 1, so the two precisions legitimately disagree about WHICH pixels of one colour still average -- each keeps
the two colours apart, which tests/test_gpu_denoise_hostile.py checks on its own.

Measured (numpy 2.2.6, x86-64; denoise_hostile.bars recomputes them wherever the tests run):
  case                  filtered share   sensitivity   8 x        to float64   4 x
  smooth-37x21          1.000            7.2e-07       5.8e-06    8.8e-07      3.5e-06
  holes-37x21           0.355            6.2e-07       5.0e-06    6.7e-07      2.7e-06
  zero_variance-37x21   1.000            4.8e-07       3.8e-06    (excluded)
  dark-37x21            1.000            6.9e-07       5.5e-06    8.2e-07      3.3e-06
  normals-37x21         1.000            6.3e-07       5.0e-06    --
  bright-37x21          1.000            5.3e-07       4.2e-06    6.7e-07      2.7e-06
  nonfinite-37x21       0.990            7.0e-07       5.6e-06    --
  smooth-259x13         1.000            1.1e-06       8.7e-06    9.2e-07      3.7e-06
  holes-259x13          0.356            6.1e-07       4.8e-06    7.9e-07      3.2e-06
  smooth-5x3            1.000            3.2e-07       2.6e-06    4.2e-07      1.7e-06
  holes-5x3             0.333            0             0          3.8e-07      1.5e-06
Every GPU bar against restate() is therefore 1e-4.  (holes-5x3: five filtered pixels; on their few weights numpy's fp32
functions and the rounded float64 ones agree bit for bit.)"""
import numpy as np
import pytest

import denoise_hostile as dh

f32 = np.float32


@pytest.fixture(scope="module", params=dh.CASES, ids=dh.case_id)
def made(request):
    case = dh.make_case(*request.param)
    rgb, var = dh.host_inputs(case)
    kept = []
    out, filt = dh.restate(rgb, var, *dh.guides(case), case.light, dh.RADIUS, case.H, kept=kept)
    return request.param, case, rgb, var, out, filt, kept


def test_the_case_is_what_it_claims(made):
    (family, W, H), c, rgb, var, out, filt, kept = made
    assert c.rows == dh.plane_rows(H) and c.rows > H and c.pos.shape == (c.rows, W, 4) and len(c.sums) == c.folds + 1 and c.folds >= 2
    # the rows past H: surfaces and no emitters by their planes, 1e30 or NaN in everything else
    assert (c.pos[H:, :, 3] == 1).all() and not c.light[H:].any()
    for p in (c.pos[H:, :, :3], c.nrm[H:], c.dif[H:], c.phg[H:], c.photon[H:]) + tuple(s[H:] for s in c.sums):
        assert (p[:, 0::2] >= f32(1e30)).all() and np.isnan(p[:, 1::2]).all()
    assert not filt[H:].any()
    share = float(filt[:H].mean())
    print(f"\n{dh.case_id((family, W, H))}: filtered share {share:.3f}")
    assert (0.2 < share < 0.95) if family == "holes" else share > 0.9
    # non-negative colours (NaN aside), so every sum of the filter is of non-negative terms
    assert not (rgb[:H] < 0).any() and not (var[:H] < 0).any()
    if family != "nonfinite":
        assert np.isfinite(rgb[:H]).all() and np.isfinite(var[:H]).all() and np.isfinite(out[:H]).all()
        assert out[~filt].tobytes() == rgb[~filt].tobytes()
    if family == "smooth":
        pos, nrm = c.pos[:H, :, :3].astype(np.float64), c.nrm[:H, :, :3].astype(np.float64)
        plane = np.abs((nrm[:, :-1] * (pos[:, 1:] - pos[:, :-1])).sum(-1)) / (0.01 * dh.RADIUS)
        assert (plane > 3).sum() == H and (plane < 1).sum() == H * (W - 2)                       # one depth step, one column wide
        assert len(np.unique(nrm.reshape(-1, 3), axis=0)) == 2                                    # one crease
        assert (c.dif[:H, 0, 0] != c.dif[:H, W - 1, 0]).all()                                     # an albedo gradient
        assert var[:H].min() > 0
    if family == "holes":
        surface = c.pos[:H, :, 3] != 0
        assert 0.35 < surface.mean() < 0.75
        y, x = c.marks["isolated"]
        assert filt[y, x] and filt[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2].sum() == 1
        assert all(filt[p] for p in c.marks["corners"])
        tenths = c.marks["emitters"]
        assert all(t.any() for t in tenths) and not (tenths[0] & tenths[1]).any() and not (tenths[1] & tenths[2]).any() and not (tenths[0] & tenths[2]).any()
        assert all((t & surface).any() and not (t & filt[:H]).any() for t in tenths)              # unfiltered by the light plane alone
        assert (c.sums[-1][:H, :, :3][~surface] == 50).all()
    if family == "zero_variance":
        assert var[:H].max() == 0 and var[:H].min() == 0
        assert len(np.unique(rgb[:H].reshape(-1, 3), axis=0)) == 2 and 0.3 < c.marks["two"].mean() < 0.7
    if family == "dark":
        total = c.dif[:H, :, :3] + c.phg[:H, :, :3]
        assert {0.0, float(f32(5e-4)), float(f32(1e-3))} <= set(np.unique(total).tolist())
        assert (total[..., 0] == f32(1e-3)).any() and (c.phg[:H, :, 0] == f32(5e-4)).any()        # 1e-3 as 5e-4 + 5e-4
        assert (total < f32(1e-3)).any(-1).mean() > 0.4                                           # pixels at the floor
        spread = total.max(-1) / np.maximum(total.min(-1), f32(1e-30))
        assert (spread >= 999).any() and total.max() == 1.0
    if family == "normals":
        zero = c.marks["zero_normal"]
        assert zero.sum() >= 5 and not c.nrm[:H, :, :3][zero].any()
        assert all((k[:H][zero]).all() for k in kept) and (kept[0][:H] == zero).all()             # sum w == 0: the restatement keeps them
        assert np.abs(out[:H][zero] - rgb[:H][zero]).max() <= 2.0 ** -22 * rgb[:H][zero].max()     # a (c / a): two roundings, no neighbour
        n = c.nrm[:H, :, :3]
        opposite = ((n[:, 1:] * n[:, :-1]).sum(-1) < -0.99)
        assert opposite.sum() > H
    if family == "bright":
        finite = rgb[:H][rgb[:H] > 0]
        assert finite.min() < 1e-6 and finite.max() > 1e5 and var[:H].max() / var[:H][var[:H] > 0].min() > 1e20
    if family == "nonfinite":
        kinds = c.marks["kinds"]
        assert set(kinds) == set(dh.KINDS) and all(len(v) == 2 for v in kinds.values())
        bad = np.zeros((c.rows, W), bool)
        for y, x in c.marks["bad"]:
            bad[y, x] = True
            assert not bad[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].sum() > 1                    # isolated: no two share a footprint at h = 1
        a = np.maximum(c.dif[..., :3] + c.phg[..., :3], f32(1e-3))
        with np.errstate(over="ignore", invalid="ignore"):
            u = rgb / a
        for y, x in kinds["inf"]:
            assert np.isposinf(rgb[y, x]).any() and not np.isnan(rgb[y, x]).any()
        for y, x in kinds["nan"]:
            assert np.isnan(rgb[y, x]).any()
        for y, x in kinds["variance"]:
            assert np.isfinite(rgb[y, x]).all() and np.isfinite(u[y, x]).all() and np.isposinf(var[y, x]).all() and all(np.isfinite(s[y, x]).all() for s in c.sums)
        for y, x in kinds["overflow"]:
            assert np.isfinite(rgb[y, x]).all() and np.isfinite(var[y, x]).all() and np.isposinf(u[y, x]).all() and (a[y, x] == f32(1e-3)).all()
        # the rule: those pixels and no others are unfiltered; the restatement's output is finite everywhere else
        assert ((c.pos[..., 3] != 0) & ~filt)[:H].tobytes() == bad[:H].tobytes()
        assert np.isfinite(out[:H][~bad[:H]]).all() and out[bad].tobytes() == rgb[bad].tobytes()
        masked = dh.make_case(family, W, H, masked=True)
        assert not masked.pos[..., 3][bad].any() and all(np.array_equal(p[~bad], q[~bad], equal_nan=True) for p, q in
                                                         zip(dh.guides(c) + (c.light, c.sums[-1]), dh.guides(masked) + (masked.light, masked.sums[-1])))
        mrgb, mvar = dh.host_inputs(masked)
        mout, _ = dh.restate(mrgb, mvar, *dh.guides(masked), masked.light, dh.RADIUS, H)
        assert mout[:H][~bad[:H]].tobytes() == out[:H][~bad[:H]].tobytes()


def test_the_bars_are_reachable(made):
    (family, W, H), c, rgb, var, out, filt, _ = made
    sens, to64 = dh.bars((family, W, H))
    print(f"\n{dh.case_id((family, W, H))}: sensitivity {sens:.2e} (x 8: {8 * sens:.2e}), restate against statement64 {to64:.2e} (x 4: {4 * to64:.2e})")
    assert 8 * sens < 1e-3
    assert max(1e-4, 8 * sens) == 1e-4                      # (as the table of the docstring says)
    want, F = dh.statement64(rgb, var, *dh.guides(c), c.light, dh.RADIUS, H)
    assert F.tobytes() == filt.tobytes()
    if family in dh.F64_FAMILIES:
        # the two references agree to a few fp32 roundings carried through five passes: far below anything a wrong weight would do
        assert 0 < to64 < 1e-5
        assert dh.rel_err(out[:H][filt[:H]], want[:H][filt[:H]]) == to64


def test_the_references_answer_to_every_parameter():
    """each argument of the two references moves their output, and both move alike: a sigma wired to the wrong term in one of them shows"""
    c = dh.make_case("smooth", 37, 21)
    rgb, var = dh.host_inputs(c)
    args = (rgb, var) + dh.guides(c) + (c.light, dh.RADIUS, c.H)
    base = dh.restate(*args)[0]
    seen = [base.tobytes()]
    for kw in (dict(levels=1), dict(levels=2), dict(sigma_l=0.5), dict(sigma_l=64.0), dict(sigma_n=0.5), dict(sigma_n=1024.0), dict(sigma_x=1e-4), dict(sigma_x=10.0)):
        a = dh.restate(*args, **kw)[0]
        names = dict(levels="levels", sigma_l="sigma_luminance", sigma_n="sigma_normal", sigma_x="sigma_position")
        b = dh.statement64(*args, **{names[k]: v for k, v in kw.items()})[0]
        assert a.tobytes() not in seen, kw
        seen.append(a.tobytes())
        assert dh.rel_err(a[:c.H], b[:c.H]) < 1e-5, kw
