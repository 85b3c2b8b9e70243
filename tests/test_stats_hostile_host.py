"""The hostile statistics cases of tests/stats_hostile.py without a GPU: every case is what it claims, the nonfinite family's broken set is
the one the rule names, the shared restatement stays within the derived bar of the independent float64 statement on every family (so the
bars are reachable without the kernel), the retire decision's tau lies in a gap far wider than the bar, evplp_plan_budgets takes the tile
figures formed under the rule and refuses the same figures formed the old way, and every mutation of the restatement fails a named check.

Worst restate-to-statement64 error / bar per family over all calls (2026-10-21; variance image / figures / tile figures), each asserted
<= 1: decades 0.699 / 0.0191 / 0.0586, late_start 0.625 / 1.9e-10 / 1.9e-10, inexact_S 0.0937 / 0.0184 / 0.0255, zero_variance 0.0933 /
0.0198 / 0.0247, emitters 0.171 / 0.00316 / 0.0295, nonfinite 0.688 / 0 / 0.1, masks 0.692 / 0.1 / 0.1."""
import numpy as np
import pytest

import stats_hostile as sh
from stats_hostile import f32, f64

CASES = sh.CASES


@pytest.fixture(scope="module")
def built():
    """every case with, per call, the host composite and both references: computed once, shared, never changed"""
    out = {}
    for key in CASES:
        case = sh.make_case(*key)
        calls = []
        for scale, ls, me in case.calls:
            comp = sh.host_composite(case, scale, ls, me)
            calls.append((scale, ls, me, comp, sh.restate(case, scale, ls, me, comp), sh.statement64(case, scale, ls, me, comp)))
        out[key] = (case, calls)
    return out


def _exact_S(case):
    cs = sh.sums_of(case)
    first, last = cs[0], cs[case.K]
    with np.errstate(all="ignore"):
        return (last - first).astype(f32).astype(f64) != last.astype(f64) - first.astype(f64)


@pytest.mark.parametrize("key", CASES, ids=sh.case_id)
def test_every_case_is_what_it_claims(built, key):
    case, calls = built[key]
    H, W = case.H, case.W
    assert case.rows == sh.plane_rows(H) and len(case.states) == case.B + 1
    for p in case.states + [case.photon, case.light]:                        # the rows past H are hostile in every uploaded plane
        assert p.shape == (case.rows, W, 4) and (p[H:, 0::2] == f32(1e30)).all() and np.isnan(p[H:, 1::2]).all()
    assert not case.photon[:H].any()
    scale, ls, me, comp, rs, ref = calls[0]
    assert scale == 1.0 / case.K and not me
    fam = case.family
    if fam == "decades":
        mean = sh.sums_of(case)[case.K].astype(f64)[..., 0].mean(0) / case.K
        assert mean.max() / mean.min() > (1e20 if (W > 5 and case.variant == 0) else 1e10)
        assert len(set(case.schedule)) > 1 and (case.variant == 0 or max(case.schedule) == 1 << 20)
        assert not ref.broken.any()
    if fam == "late_start":
        cs = list(sh.sums_of(case).values())
        vanish = case.marks["vanish"]
        assert vanish.any() or W < 4
        per_it = (cs[-1].astype(f64) - cs[0]) / case.K
        assert (cs[0][~vanish] >= 2.0 ** 22 * per_it[~vanish]).all()         # tracking starts on sums of about 2^24 iterations
        for a, b in zip(cs, cs[1:]):
            assert (a[vanish] == b[vanish]).all()                            # the increments vanished: D = 0 in every fold
            d, ulp = (b - a)[~vanish].astype(f64), np.spacing(a[~vanish]).astype(f64)
            assert (d > 0).mean() > 0.3 and ((d == 0).any() or W == 5) and (d % ulp == 0).all() and (d < 64 * ulp).all()      # ... or are a few ulps of the sum, or none
        assert (rs.v[vanish] == 0.0).all() and (rs.var[vanish] == 0.0).all() and (ref.var[vanish] == 0.0).all()
        print(f"{sh.case_id(key)}: {int(vanish.sum())} pixels with D = 0 in every fold, v exactly 0")
    if fam == "inexact_S":
        cs = sh.sums_of(case)
        assert (np.log2(np.abs(cs[case.K].astype(f64)) / np.abs(cs[0].astype(f64))) >= 30).all() and (cs[0] < 0).any() and (cs[0] > 0).any()
        rounded = _exact_S(case)
        neg = rs.v < 0
        print(f"{sh.case_id(key)}: S rounds in {int(rounded.sum())} of {rounded.size} channels; the clamp decides {int(neg.sum())}")
        assert rounded.mean() > 0.9 and 0.05 < neg.mean() < 0.95
        assert (np.abs(rs.v) <= ref.bar / (2.0 * f64(f32(scale)) ** 2 * case.K) + ref.var / (f64(f32(scale)) ** 2 * case.K)).all()
    if fam == "zero_variance":
        exact = case.marks["exact"]
        assert (rs.v[exact] == 0.0).all() and (ref.var[exact] == 0.0).all()
        other = rs.v[~exact]
        print(f"{sh.case_id(key)}: {int(exact.sum()) * 3} exact zeros; d = 0.1: {int((other < 0).sum())} negative, {int((other > 0).sum())} positive, {int((other == 0).sum())} zero")
        assert (other < 0).any() and (other > 0).any()
    if fam == "emitters":
        kind = case.marks["kind"]
        lx = case.light[:H, :, 0]
        assert ((lx[kind == 1] * f32(1e-20)) == 0).all() and (lx[kind == 1] > 0).all()
        by = {(ls_, me_): r for _, ls_, me_, _, _, r in calls}
        for ls_ in (1.0, 1e-20, 0.0, -1.0):
            assert not by[(ls_, False)].emitter.any()
            want = {1.0: (kind == 1) | (kind == 4), 1e-20: kind == 4, 0.0: np.zeros_like(kind, bool), -1.0: kind == 2}[ls_]
            assert np.array_equal(by[(ls_, True)].emitter, want), ls_
            assert np.array_equal(by[(ls_, True)].broken, kind == 3)         # a NaN light: the composite is NaN whatever the scale
    if fam in ("nonfinite", "masks"):
        m = case.marks
        per_tile = sh.broken_per_tile(ref.broken)
        want = np.zeros_like(per_tile)
        one = m["one"]; want[one[0] // 8, one[1] // 8] += 1
        if m["all_tile"] is not None:
            ty, tx = m["all_tile"]
            want[ty, tx] = sh.in_image_per_tile(W, H)[ty, tx]
            for k in ("col", "row", "replaced"):
                want[m[k][0] // 8, m[k][1] // 8] += 1
            assert m["col"][1] // 8 == (W - 1) // 8 and W % 8 and m["row"][0] // 8 == (H - 1) // 8 and H % 8
        assert np.array_equal(per_tile, want), (per_tile, want)
        assert (per_tile == 1).any() and (m["all_tile"] is None or per_tile[m["all_tile"]] == sh.in_image_per_tile(W, H)[m["all_tile"]])
        for k in ("variance", "overflow"):
            assert not ref.broken[m[k]]
        y, x = m["variance"]
        assert (rs.var[y, x] > sh.FLT_MAX).all() and np.isfinite(rs.var[y, x]).all() and np.isinf(sh.to32(rs.var)[y, x]).all()
        y, x = m["overflow"]
        assert (rs.var[y, x] == 0).all() and abs(np.log2(comp[y, x, 0]) - 120) < 0.01
        if m["replaced"] is not None:
            y, x = m["replaced"]
            assert np.isfinite(comp[y, x]).all() and rs.v[y, x, 0] == np.inf
        if fam == "masks":
            keep = case.mask[::-1].any(-1)
            if case.variant == 0:
                assert not keep.any()
            if case.variant == 1:
                assert np.array_equal(keep, ref.broken)
            if case.variant == 2:
                assert keep.any() and not (keep & ref.broken).any() and set(np.unique(case.mask)) == {0, 1} and not case.mask[..., 0].any()
                assert not np.array_equal(keep, keep[::-1])


@pytest.mark.parametrize("key", [k for k in CASES if k[0] in ("nonfinite", "masks")], ids=sh.case_id)
def test_nonfinite_cases_have_the_broken_set_the_rule_names(built, key):
    """the rule, applied to the restatement's own v and den, against the set read off the sums (statement64) -- at every scale: 1e20 takes the
    2^120 composite and the 1e20 sums to Inf, and 0 times an infinite sum is NaN"""
    case, calls = built[key]
    for scale, ls, me, comp, rs, ref in calls:
        by_rule = np.isnan(rs.rel)
        assert np.array_equal(by_rule, ref.broken), (scale, np.argwhere(by_rule != ref.broken))
        assert np.array_equal(np.isnan(rs.num), ref.broken)
        nan_figs = [bool(np.isnan(f)) for f in rs.figs]
        keep = np.ones_like(by_rule) if case.mask is None else case.mask[::-1].any(-1)
        assert nan_figs == [True, True, bool((keep & by_rule).any())], (scale, nan_figs)
        # the variance image keeps its bytes: a NaN v reads 0 (NaN only where an infinite v meets a scale of exactly 0), never negative
        var32 = sh.to32(rs.var)
        assert np.array_equal(np.isnan(var32), np.isinf(rs.v) & (f32(scale) == 0)) and not (var32 < 0).any()
        assert (var32[np.isnan(rs.v)] == 0).all()
    m = case.marks
    scale20 = [c for c in calls if c[0] == 1e20 and not c[2]][0]
    assert scale20[5].broken[m["overflow"]] and scale20[5].broken[m["variance"]]
    if case.mask is not None and case.variant == 0:
        assert all(c[4].figs[2] == 0.0 for c in calls)                       # keep nothing: the third figure is 0


def ratios(case, calls, of=None):
    """the worst error / bar of `of` (default: the restatement) against statement64 over the calls: variance image, figures, tile figures"""
    rv = rf = rt = 0.0
    for scale, ls, me, comp, rs, ref in calls:
        got = rs if of is None else of(case, scale, ls, me, comp)
        rv = max(rv, sh.variance_ratio(sh.to32(got.var), ref))
        rf = max(rf, sh.worst_ratio(got.figs, ref.figs, ref.fig_bars))
        rt = max(rt, sh.worst_ratio(got.tiles, ref.tiles, ref.tile_bars))
    return rv, rf, rt


def test_restatement_within_the_derived_bar_of_statement64(built):
    worst = {}
    for key in CASES:
        case, calls = built[key]
        r = ratios(case, calls)
        w = worst.setdefault(case.family, [0.0, 0.0, 0.0])
        for i in range(3):
            w[i] = max(w[i], r[i])
    for fam, w in worst.items():
        print(f"restate / statement64, worst error / bar, {fam}: variance {w[0]:.3g}, figures {w[1]:.3g}, tiles {w[2]:.3g}")
    for fam, w in worst.items():
        assert max(w) <= 1.0, (fam, w)
    assert set(worst) == set(sh.FAMILIES)


def test_mutant_without_a_mutation_is_the_restatement(built):
    for key in CASES:
        case, calls = built[key]
        for scale, ls, me, comp, rs, ref in calls:
            mt = sh.mutant(case, scale, ls, me, comp)
            assert sh.same_nan(sh.to32(mt.var), sh.to32(rs.var)) and np.array_equal(mt.tiles, rs.tiles)
            assert all(sh.figure_ratio(a, b, 0.0) == 0.0 for a, b in zip(mt.figs, rs.figs)), (key, scale, mt.figs, rs.figs)


# Which check catches which mutation of the restatement, and on which case.  "variance64" / "figures64" / "tiles64": the derived bar against
# statement64 (test_restatement_within_the_derived_bar_of_statement64; on the GPU test_gpu_stats_hostile.py test_plain_context).  "variance_rule":
# the variance image is never negative and a NaN v reads 0 (test_nonfinite_cases_have_the_broken_set_the_rule_names).  "bytes": the variance
# image differs from the restatement's in its bytes, which the kernel's image is compared with on the GPU (test_plain_context) -- taking S in
# double is CLOSER to statement64, so only the bytes can show it.
CAUGHT_BY = {
    "no_clamp": ("variance_rule", ("inexact_S", 37, 21, 0)),
    "S_double": ("bytes", ("inexact_S", 37, 21, 0)),
    "kj_for_K": ("figures64", ("decades", 37, 21, 0)),
    "B_for_B1": ("variance64", ("decades", 37, 21, 0)),
    "mask_not_flipped": ("figures64", ("masks", 37, 21, 2)),
    "emitter_without_scale": ("figures64", ("emitters", 37, 21, 0)),
    "broken_counted": ("tiles64", ("nonfinite", 37, 21, 0)),
    "broken_num_zero": ("figures64", ("nonfinite", 37, 21, 0)),
}


@pytest.mark.parametrize("mut", sh.MUTATIONS)
def test_every_mutation_fails_its_named_check(built, mut):
    check, key = CAUGHT_BY[mut]
    case, calls = built[key]
    of = lambda c, s, ls, me, comp: sh.mutant(c, s, ls, me, comp, mut)
    rv, rf, rt = ratios(case, calls, of)
    if check == "variance64":
        assert rv > 1.0, rv
    elif check == "figures64":
        assert rf > 1.0, rf
    elif check == "tiles64":
        assert rt > 1.0, rt
    elif check == "variance_rule":
        assert any((sh.to32(of(case, *c[:4]).var) < 0).any() for c in calls)
    elif check == "bytes":
        scale, ls, me, comp, rs, ref = calls[0]
        assert sh.to32(of(case, scale, ls, me, comp).var).tobytes() != sh.to32(rs.var).tobytes()
    print(f"{mut}: caught by {check} on {sh.case_id(key)} (variance {rv:.3g}, figures {rf:.3g}, tiles {rt:.3g})")


# zero_variance and inexact_S are left out: their v is a rounding by construction, so no tau separates their tiles by more than the bar; so
# is the decades variant whose one batch of 2^20 iterations holds nearly all of Q (v is a 1e-6 remainder of Q - S^2 / K, a bar's size)
TAU_FAMILIES = ("decades", "late_start", "emitters", "nonfinite", "masks")
TAU_CASES = [k for k in CASES if k[0] in TAU_FAMILIES and sh.tiles_of(k[1], k[2]) != (1, 1) and k != ("decades", 37, 21, 1)]


@pytest.mark.parametrize("key", TAU_CASES, ids=sh.case_id)
def test_tau_lies_in_a_gap_far_wider_than_the_bar(built, key):
    case, calls = built[key]
    scale, ls, me, comp, rs, ref = calls[0]
    tau, gap, bar = sh.pick_tau(ref.tiles, ref.tile_bars)
    print(f"{sh.case_id(key)}: tau {tau:.4g} in a gap of {gap:.4g}, {gap / bar if bar else np.inf:.3g} bars")
    assert gap >= 100.0 * bar and gap > 0
    assert np.array_equal(rs.tiles <= tau, ref.tiles <= tau)                 # the restatement decides as the statement does


@pytest.mark.parametrize("key", CASES, ids=sh.case_id)
def test_the_planner_takes_the_figures_of_the_rule_and_refuses_the_old_ones(evplp, built, key):
    """the handoff that broke: one NaN pixel made its tile's figure NaN and evplp_plan_budgets refused the whole plan"""
    case, calls = built[key]
    for scale, ls, me, comp, rs, ref in calls:
        n_t = np.full(rs.tiles.shape, case.K, np.int32)
        assert np.isfinite(rs.tiles).all() and (rs.tiles >= 0).all()
        plan = evplp.plan_budgets(rs.tiles, n_t, 16, 1, 0.0, 1.0)
        assert plan.size == rs.tiles.size and (plan >= 1).all() and (plan <= 16).all()
        old, old_rel = sh.old_tiles(case, scale, ls, me, comp)
        if np.isnan(old_rel).any():
            assert np.isnan(old).any()
            with pytest.raises(evplp.EvplpError):
                evplp.plan_budgets(old, n_t, 16, 1, 0.0, 1.0)
        elif not ref.broken.any():
            assert np.array_equal(old, ref.tiles) or np.allclose(old, rs.tiles, rtol=1e-12, atol=0)
    scale, ls, me, comp, rs, ref = calls[0]
    if case.family in ("nonfinite", "masks"):
        old, old_rel = sh.old_tiles(case, scale, ls, me, comp)
        # defect 1: the Inf pixel read as converged -- its old rel is 0 (or NaN), never the noise it hides
        y, x = case.marks["one"]
        assert old_rel[y, x] == 0.0 or np.isnan(old_rel[y, x])
        assert np.isnan(old).any() == bool(np.isnan(old_rel).any())
