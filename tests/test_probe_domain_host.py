"""No GPU: the inputs and references of tests/probe_domain.py, checked on their own (caps, coverage, what each hostile family visits), and
evplp_probe_pair -- the host twin -- held to them under K_ORACLE_PROBE with hw_pow = False.  test_gpu_probe_domain.py runs the same cases
through probe_gather_kernel.  The twin has visibility 1: it is expected to carry the term of every pair that casts a ray, lit or not."""
import numpy as np
import pytest

import oracle_api as oa
import probe_domain as pd
import probe_restate as pr
import shading_domain as sd

F = np.float32
K = pd.K_ORACLE_PROBE


def twin(evplp, rec, X):
    return np.stack([evplp.probe_pair(rec, x, pd.MIN_DISTANCE) for x in X]).astype(np.float64)


@pytest.fixture(scope="module")
def floor(oracle):
    return oa.Scene(sd.floor_scene())


@pytest.fixture(scope="module")
def hostile(oracle):
    return pd.hostile_reference(oa.Scene(pd.hostile_scene()), K, False)


def test_probe_pair_over_the_material_domain_with_the_oracles_visibility(evplp, floor):
    recs, names = pd.domain_records()
    und, facing_pairs, rays, aside, worst, seen = [], 0, 0, 0, 0.0, {}
    for k, name in enumerate(names):
        X, kinds = pd.positions_for(recs[k])
        assert len(X) == 369
        ref = pd.Reference(floor, sd.only_slot(recs, k, 1), X, per_path=pd.P, K=K, hw_pow=False)
        assert ref.walked[0][kinds != "at_vpl"].all() and not ref.walked[0][kinds == "at_vpl"].any(), name
        got = twin(evplp, recs[k].astype(evplp.RECORD_DTYPE), X)
        worst = max(worst, pd.check_single(got, None, ref, ref.facing[0], name, kinds))
        assert (got[kinds == "behind"] == 0.0).all() and (got[kinds == "at_vpl"] == 0.0).all(), name
        if name in sd.DARK_VPLS:                   # (in front of them the other two do light a probe: only the flux decides everywhere)
            assert (got[kinds == "grid"] == 0.0).all() and (name != "zero_flux" or (got == 0.0).all()), name
        und.append(int((ref.facing[0] & ~ref.decided[0]).sum())); facing_pairs += int(ref.facing[0].sum())
        rays += len(ref.rays); aside += int(ref.aside_rays.sum())
        lit = np.abs(got).sum(axis=(1, 2)) > 0
        for kind in np.unique(kinds):
            seen[kind] = seen.get(kind, 0) + int(lit[kinds == kind].sum())
        seen["occluded"] = seen.get("occluded", 0) + int((ref.facing[0] & ~ref.lit[0]).sum())
        if np.any(recs[k]["rho_s"] != 0) and ref.facing[0][kinds == "on_lobe"].any():
            lam = pr.pair_f64(recs[k], X, pd.MIN_DISTANCE)[2]
            seen["lobe_term"] = seen.get("lobe_term", 0) + int((lam[kinds == "on_lobe"] > 0).any() or recs[k]["phong_exp"] == 0)
    caps = sd.check_caps(und, facing_pairs)
    pd.say(f"twin, domain: worst error / bar = {worst:.3f} over {len(names)} records, {facing_pairs} facing pairs, {rays} rays ({aside} set aside); "
           f"undecided: worst record {caps[0]}, all {caps[1]}; by kind {seen}")
    assert facing_pairs == rays and aside <= 0.005 * rays
    assert seen["grid"] > 5000 and seen["inside_min_distance"] > 20 and seen["on_lobe"] > 20 and seen["lobe_flank"] > 20 and seen["lobe_term"] >= 8
    assert seen["behind"] == 0 and seen["at_vpl"] == 0
    assert seen["occluded"] >= 10, "some probes lie under the floor: the kernel's walk has something to find"


def summed_twin(evplp, recs, X, paths):
    """the kernel's sum restated with the twin's terms: slot order, float32, then the division"""
    acc = np.zeros((len(X), 9, 3), F)
    for k in np.nonzero(recs["flags"] & 1)[0]:
        acc = (acc + np.stack([evplp.probe_pair(recs[k], x, pd.MIN_DISTANCE) for x in X])).astype(F)
    return (acc / F(paths)).astype(F)


def test_the_summed_case_on_the_grid(evplp, floor):
    recs, names = pd.domain_records()
    X = pd.grid_probes(recs[0])
    assert len(X) == 360
    ref = pd.Reference(floor, recs, X, per_path=pd.P, K=K, hw_pow=False)
    assert ref.aside_rays.sum() == 0 and len(ref.slots) == len(names) == 37
    _, _, lit, und = ref.expect(pd.NPATHS)
    sd.check_caps([int(u) for u in (ref.lit & ~ref.decided).sum(1)], int(lit.sum()))
    assert np.array_equal(ref.lit, ref.facing), "on and above the floor nothing occludes: the twin's visibility 1 is the scene's"
    got = np.zeros(len(X), evplp.PROBE_SH_DTYPE)
    got["c"] = summed_twin(evplp, recs.astype(evplp.RECORD_DTYPE), X, pd.NPATHS); got["lit"] = lit
    pd.check_values(got, ref, pd.NPATHS, "twin, 37 records summed on the grid")
    assert lit.min() >= 10


def test_the_hostile_families_visit_what_they_are_built_for(hostile):
    rec, names, slots, X, fam, lab, refs = hostile
    ok = pd.valid_probes(X)
    assert ok.sum() == len(X) - 3 and list(fam[~ok]) == ["invalid"] * 3
    at = np.cumsum(ok) - 1                                   # index among the valid probes
    want = pd.expected_walk(names, fam, lab)
    assert sum(want.values()) >= 40 and sum(not w for w in want.values()) >= 20
    for (name, i), w in want.items():
        ref = refs[slots[names.index(name)]]
        assert ref.walked[0][at[i]] == w and ref.facing[0][at[i]] == w, (name, lab[i], w)
    und, facing = [], 0
    for k, ref in refs.items():
        assert ref.aside_rays.sum() == 0 and (ref.occluded_rays == 0).all(), "free space: the oracle's two walks see no occluder on any ray"
        assert np.isfinite(ref.term).all() and np.abs(ref.term).max() < 1e30
        und.append(int((ref.facing[0] & ~ref.decided[0]).sum())); facing += int(ref.facing[0].sum())
    i = [at[j] for j in np.nonzero(fam == "lobe_cut")[0]]
    for name in ("lobe_cut_e1000", "lobe_cut_e0"):
        cut = refs[slots[names.index(name)]]
        assert list(cut.decided[0][i]) == [True, True, False, False, True] and cut.facing[0][i].all(), name
    on = pr.pair_f64(rec[slots[names.index("lobe_cut_e0")]], X[ok][i], pd.MIN_DISTANCE)[0][:, 0, 0]
    assert on[4] > 1.5 * on[1] and abs(on[0] - on[4]) < 1e-3 * on[0], "the lobe is on 5e-6 above the cut as it is 1e-5 above it, and off below"
    assert sum(und) == 4 and facing > 250, "the pairs 1e-7 from the lobe cut are undecided by construction; nothing else is"
    # the walked rays are rays evplp_trace_occluded accepts (include/evplp.h: the direction's largest component in [2^-64, 2^64])
    for ref in refs.values():
        big = np.abs(ref.rays[:, 4:7]).max(axis=1)
        assert ((big >= F(2.0 ** -64)) & (big <= F(2.0 ** 64))).all()


def test_probe_pair_on_the_hostile_pairs(evplp, hostile):
    rec, names, slots, X, fam, lab, refs = hostile
    ok = pd.valid_probes(X)
    r32 = rec.astype(evplp.RECORD_DTYPE)
    worst = {}
    for name, k in zip(names, slots):
        ref = refs[k]
        got = twin(evplp, r32[k], X[ok])                     # (check_single: finite everywhere, exactly 0 off the walked pairs)
        pd.check_single(got, None, ref, ref.facing[0], name, lab[ok])
        ratio = np.where((ref.facing[0] & ref.decided[0])[:, None, None], np.abs(got - ref.term[0]) / ref.bar[0], 0.0).max(axis=(1, 2))
        for f in np.unique(fam[ok]):
            worst[f] = max(worst.get(f, 0.0), float(ratio[fam[ok] == f].max()))
        near = np.isin(fam[ok], ("near_walked",)) & ref.facing[0]
        assert (np.abs(got[near]).sum(axis=(1, 2)) > 0).all(), (name, "a walked pair inside min_distance carries its clamped term")
    pd.say("twin, hostile: worst error / bar by family " + ", ".join(f"{f} {w:.3f}" for f, w in sorted(worst.items())))
