"""probe_gather_kernel (evplp_gather_probes, once through its device form) against float64 over the material domain and on the hostile
pairs of tests/probe_domain.py -- the cases test_probe_domain_host.py holds the host twin to, here under
shading_domain.bar(term, kappa, lam, K_GPU_PROBE = 2 K_ORACLE_PROBE, hw_pow=True).  What in the kernel each is built to catch:
  the 37 record classes one at a time, lobes visited on the axis and on the flank: the rho_s = 0 skip (rsx_zero lights two channels), a
      wrong value out of the e = 0 branch, the sign of reflect(-fdir, n) (a flipped axis moves the lobe off the on_lobe probes: a
      factor, not a rounding), and the field offsets of the scalar record fetch (rd, rs and e differ per class and channel)
  the e = 0 lobe 5e-6 above the cut: the cut is 1e-6 and not the 1e-5 of the photon shader
  inside_min_distance and near_walked: max(dist2, min_distance^2) (without it 1 / dist2 of 2^-40 .. 2^-124)
  near_edge, near_below, far_edge: the dist2 test of include/evplp.h -- exact zeros, lit 0, never a non-finite byte, and the host
      twin's decision pair for pair
  unusable slots holding NaN, inf and 1e30: the flags test comes before any arithmetic on the slot
Every ray the kernel walks is also given to evplp_trace_occluded, which must answer 0 or 1 -- never 2, an invalid ray -- and what the
oracle's brute force answers.  (Taking the e = 0 branch away altogether changes no bit: exp2(0 log2 d) is 1 for every d above the cut.
No test can tell, and none needs to.)

The worst error / bar each test prints, measured on an MI355X on 2026-10-21, is in DESIGN section 6d; the file runs in about 2.5 s."""
import numpy as np
import pytest

import oracle_api as oa
import probe_domain as pd
import shading_domain as sd

pytestmark = pytest.mark.gpu

F = np.float32
W, H = sd.W, sd.H                    # the contexts' frame: nothing renders
MD = pd.MIN_DISTANCE


def context(evplp, scene, paths=pd.NPATHS):
    c = evplp.Context(W, H, paths, paths, pd.P, deterministic=True)
    scene.upload(c)
    return c


def put(evplp, c, rec):
    c.upload(evplp.BUF_RECORDS, rec.astype(evplp.RECORD_DTYPE))


def check_rays(c, ref, what):
    """the header's sentence: every ray the kernel walks is one evplp_trace_occluded accepts, and it answers what the brute force does"""
    occ = c.trace_occluded(ref.rays)
    assert occ.max(initial=0) <= 1, (what, "an invalid ray among the walked ones", ref.rays[occ > 1][:4])
    keep = ~ref.aside_rays
    assert np.array_equal(occ[keep], ref.occluded_rays[keep]), what


@pytest.fixture(scope="module")
def floor():
    return sd.floor_scene()


@pytest.fixture(scope="module")
def hscene():
    return pd.hostile_scene()


@pytest.fixture(scope="module")
def hostile(oracle, hscene):
    return pd.hostile_reference(oa.Scene(hscene), pd.K_GPU_PROBE, True)


# ---- 1: the material domain
def test_every_record_class_alone_against_float64(evplp, oracle, floor):
    recs, names = pd.domain_records()
    osc = oa.Scene(floor)
    worst, und, lit_pairs, rays, aside, occluded = 0.0, [], 0, 0, 0, 0
    with context(evplp, floor) as c:
        for k, name in enumerate(names):
            X, kinds = pd.positions_for(recs[k])
            one = sd.only_slot(recs, k, 1)
            ref = pd.Reference(osc, one, X, per_path=pd.P)
            put(evplp, c, one)
            got = c.gather_probes(X, pd.NPATHS, pd.P, MD)
            worst = max(worst, pd.check_single(got["c"].astype(np.float64) * pd.NPATHS, got["lit"], ref, ref.lit[0], name, kinds))
            check_rays(c, ref, name)
            if name in sd.DARK_VPLS:
                assert (got["c"][kinds == "grid"] == 0).all() and (name != "zero_flux" or (got["c"] == 0).all()), name
            assert (got["c"][(kinds == "behind") | (kinds == "at_vpl")] == 0).all() and (got["lit"][(kinds == "behind") | (kinds == "at_vpl")] == 0).all(), name
            und.append(int((ref.lit[0] & ~ref.decided[0]).sum())); lit_pairs += int(ref.lit[0].sum())
            rays += len(ref.rays); aside += int(ref.aside_rays.sum()); occluded += int((ref.facing[0] & ~ref.lit[0]).sum())
    caps = sd.check_caps(und, lit_pairs)
    pd.say(f"kernel, domain: worst error / bar = {worst:.3f} over {len(names)} records, {rays} rays ({aside} set aside, {occluded} occluded), "
           f"{lit_pairs} lit pairs; undecided: worst record {caps[0]}, all {caps[1]}")
    assert aside <= 0.005 * rays and lit_pairs > 10000 and occluded >= 10


def test_all_records_summed_on_the_grid(evplp, oracle, floor):
    recs, names = pd.domain_records()
    X = pd.grid_probes(recs[0])
    ref = pd.Reference(oa.Scene(floor), recs, X, per_path=pd.P)
    assert ref.aside_rays.sum() <= 0.005 * len(ref.rays)
    with context(evplp, floor) as c:
        put(evplp, c, recs)
        got = c.gather_probes(X, pd.NPATHS, pd.P, MD)
        check_rays(c, ref, "summed")
    lit = pd.check_values(got, ref, pd.NPATHS, "kernel, 37 records summed on the grid")
    assert lit.min() >= 10 and np.isfinite(got["c"]).all()


# ---- 2: hostile pairs
def test_hostile_pairs_follow_the_dist2_rule_and_stay_finite(evplp, hscene, hostile):
    rec, names, slots, X, fam, lab, refs = hostile
    ok = pd.valid_probes(X)
    r32 = rec.astype(evplp.RECORD_DTYPE)
    worst = {}
    with context(evplp, hscene) as c:
        for name, k in zip(names, slots):
            ref = refs[k]
            put(evplp, c, sd.only_slot(rec, k, 1))
            got = c.gather_probes(X, pd.NPATHS, pd.P, MD)
            assert np.isfinite(got["c"][ok]).all(), (name, "a probe with finite coordinates received a non-finite byte", lab[ok][~np.isfinite(got["c"][ok]).all(axis=(1, 2))])
            assert (got["c"][~ok] == 0).all() and (got["lit"][~ok] == -1).all(), name
            cc = got["c"][ok].astype(np.float64) * pd.NPATHS
            pd.check_single(cc, got["lit"][ok], ref, ref.lit[0], name, lab[ok])
            assert np.array_equal(ref.lit[0], ref.facing[0]), "free space: every walked pair is lit"
            check_rays(c, ref, name)
            if "flux" not in name:                  # (unit flux: a walked pair's term is not 0 even at 2^63, so the twin's decision shows)
                tw = np.stack([evplp.probe_pair(r32[k], x, MD) for x in X[ok]])
                assert np.array_equal((tw != 0).any(axis=(1, 2)), got["lit"][ok] == 1), (name, "the kernel and evplp_probe_pair skip the same pairs")
            ratio = np.where((ref.lit[0] & ref.decided[0])[:, None, None], np.abs(cc - ref.term[0]) / ref.bar[0], 0.0).max(axis=(1, 2))
            for f in np.unique(fam[ok]):
                worst[f] = max(worst.get(f, 0.0), float(ratio[fam[ok] == f].max()))
    pd.say("kernel, hostile: worst error / bar by family " + ", ".join(f"{f} {w:.3f}" for f, w in sorted(worst.items())))


def test_unusable_slots_have_no_effect_whatever_they_hold(evplp, hscene, hostile):
    rec, names, slots, X, fam, lab, refs = hostile
    variants = pd.filler_variants(rec)
    with context(evplp, hscene) as c:
        got = {}
        for name, r in variants.items():
            put(evplp, c, r)
            got[name] = c.gather_probes(X, pd.NPATHS, pd.P, MD)
    assert got["zero"]["lit"].max() >= 10 and np.isfinite(got["zero"]["c"]).all()
    for name in ("nan", "inf", "1e30"):
        assert got[name].tobytes() == got["zero"].tobytes(), name


# ---- 3: placement in the wave and the slice
def test_a_hostile_probes_bytes_do_not_depend_on_its_lane_or_its_neighbours(evplp, hscene, hostile):
    import torch
    rec, names, slots, X, fam, lab, refs = hostile
    src = pd.wave_batch(X, fam)
    with context(evplp, hscene) as c:
        put(evplp, c, rec)
        got = c.gather_probes(X[src], pd.NPATHS, pd.P, MD)
        dev = c.gather_probes(torch.from_numpy(X[src]).cuda(), pd.NPATHS, pd.P, MD)
        c.synchronize()
        assert dev.cpu().numpy().tobytes() == got.tobytes(), "the device form"
        for i in np.unique(src):
            alone = c.gather_probes(X[i:i + 1], pd.NPATHS, pd.P, MD)
            for at in np.nonzero(src == i)[0]:
                assert got[at:at + 1].tobytes() == alone.tobytes(), (lab[i], int(at))
    ok = pd.valid_probes(X[src])
    assert np.isfinite(got["c"][ok]).all() and (got["lit"][~ok] == -1).all() and (got["c"][~ok] == 0).all()
    assert got["lit"].max() >= 10


def test_a_record_alone_in_any_slice_gives_the_same_bytes(evplp, oracle, hscene, hostile):
    rec, names, slots, X, fam, lab, refs = hostile
    glossy = rec[slots[names.index("glossy_+z")]]
    probes = pd.slice_probes()
    ok = pd.valid_probes(probes)
    assert len(probes) == 70
    got = []
    with context(evplp, hscene, pd.SLICE_PATHS) as c:
        for place in pd.SLICE_PLACES:
            put(evplp, c, pd.slice_records(oa.RECORD_DTYPE, glossy, place))
            got.append(c.gather_probes(probes, pd.SLICE_PATHS, pd.P, MD))
    for place, g in zip(pd.SLICE_PLACES, got):
        assert g.tobytes() == got[0].tobytes(), place              # 0 + term is exact, an absent slice adds zeros
    one = np.zeros(pd.P, oa.RECORD_DTYPE); one[0] = glossy
    ref = pd.Reference(oa.Scene(hscene), one, probes[ok], per_path=pd.P)
    g = got[0][ok]
    assert np.array_equal(g["lit"], ref.lit[0].astype(F)) and ref.lit[0].sum() > 25 and not ref.aside_rays.any()
    term = ref.term[0] / pd.SLICE_PATHS
    bar = ref.bar[0] / pd.SLICE_PATHS + 2.0 ** -24 * np.abs(term)          # one rounding more: the division by 288
    err = np.abs(g["c"].astype(np.float64) - term)
    on = (ref.lit[0] & ref.decided[0])[:, None, None]
    pd.say(f"kernel, slices: worst error / bar = {float(np.where(on, err / bar, 0.0).max()):.3f} over {int(ref.lit[0].sum())} lit pairs")
    assert (np.where(on, err, 0.0) <= bar).all() and (g["c"][~ref.lit[0]] == 0).all() and np.isfinite(got[0]["c"]).all()
