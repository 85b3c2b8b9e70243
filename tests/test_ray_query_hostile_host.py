"""No GPU needed: the hostile ray batches of ray_hostile.py and their references, checked on their own.

The device tests (test_gpu_ray_query_hostile.py) compare byte for byte only the rays that the references alone call decidable, so the
share set aside is a condition on the inputs and is asserted here, per (scene, kind), where no device can bend it.  The other tests
show that every kind does what it is for: it hits and misses, the tie pairs are hit, no triangle without area ever wins, the far rays
aimed a few ulps inside a corner or an outline mostly hit, a direction scaled by a power of two keeps its winner."""
import numpy as np
import pytest

import ray_hostile as rh
from test_gpu_ray_query import brute_closest, brute_table

F = np.float32

# One (scene, kind) lies beyond what fp32 rays can address, and the cap is not asserted for it: the soup moved to (4000, -3000, 2500) has
# S = 4010, so far 1e4 puts the origins 4e7 away, past 2^24, where an origin's ulp is 4 units and a unit direction's rounding moves the
# ray by 2.4 units at the scene -- on a soup of triangles no larger than 3.  The triangle test then sees every corner moved by up to 2
# units and its winners are unrelated to the exact ray (93 of 600 set aside, 15 %; measured on the references alone).  It is the regime
# the far kinds stop short of on the other scenes (R = 1e6 there).  The rays stay in the batch and the device is held to the same rule on them.
BEYOND_FP32 = {("soup far away", "far 10000")}


def say(*a):
    print("[hostile rays]", *a, flush=True)


@pytest.fixture(scope="module")
def batches(oracle):
    return {name: rh.Hostile(rh.make_scene(name)) for name in rh.SCENES}


def kinds_of(b):
    return [k for k in dict.fromkeys(b.kinds) if k not in rh.INVALID_KINDS]


def test_each_batch_has_4096_rays_of_every_kind_and_the_scenes_stay_small(batches):
    for name, b in batches.items():
        assert b.rays.shape == (rh.N_RAYS, 8) and b.V.shape[0] - b.light[1] <= 700, name
        ks = set(kinds_of(b))
        want = {"near"} | {f"far {R:g}" for R in rh.FAR_R} | {f"scaled d 2^{e}" for e in rh.SCALES} | ({"in plane"} if name in ("flat", "room") else set())
        assert ks == want, (name, ks)
        assert set(b.kinds[b.invalid]) == set(rh.INVALID_KINDS) | set(rh.HOSTILE_INVALID) and len(b.invalid) == 10 + 2 * rh.N_SCALED
        # the far origins are where they are meant to be, and the scaled directions are exact powers of two of their base
        for R in rh.FAR_R:
            r = b.rays[b.kinds == f"far {R:g}"]
            centre = 0.5 * (b.lo + b.hi)
            dist = np.linalg.norm(r[:, 0:3].astype(np.float64) - centre, axis=1)
            assert (np.abs(dist / (R * b.S) - 1.0) < 2.0 / R + 1e-6).all(), (name, R)
    soup = batches["soup far away"]
    assert soup.S == pytest.approx(4010.0, rel=1e-3) and np.linalg.norm(soup.hi - soup.lo) < 20.0, "the largest coordinate governs S there, not the diagonal"


def test_the_share_set_aside_stays_under_the_cap_for_every_scene_and_kind(batches):
    worst = {}
    for name, b in batches.items():
        for k in kinds_of(b):
            m = b.kinds == k
            n = [int(b.aside[f][m].sum()) for f in (0, 1, 2)]
            share = max(n) / m.sum()
            say(f"{name:14s} {k:16s} {int(m.sum()):5d} rays, set aside {n} ({100 * share:.2f} %)")
            if (name, k) in BEYOND_FP32:
                assert np.abs(b.rays[m, 0:3]).max() > 2.0 ** 24, "the exemption is for origins fp32 no longer resolves to a unit"
                continue
            worst[(name, k)] = share
    over = {k: v for k, v in worst.items() if v > rh.CAP}
    assert not over, over


def test_every_kind_hits_and_misses(batches):
    for name, b in batches.items():
        for k in kinds_of(b):
            m = b.kinds == k
            share = float((b.brute[0]["triangle"][m] >= 0).mean())
            say(f"{name:14s} {k:16s} hit share {share:.3f}")
            if (name, k) == ("flat", "in plane"):
                # every triangle a ray in the plane z = 0 could reach lies in that plane: n . d is an exact zero, the test divides by it
                # and accepts nothing.  What the kind is for there is the walk through boxes without thickness, and a miss from every ray
                assert share == 0.0
                continue
            assert 0.2 <= share <= 0.98, (name, k, share)
        assert (b.brute[2]["triangle"] >= 0).any() and (b.brute[1]["triangle"] != b.brute[0]["triangle"]).any(), name


def test_tie_pairs_report_the_lower_index_and_no_triangle_without_area_wins(batches):
    for name, b in batches.items():
        for f in (0, 1, 2):
            w = b.brute[f]["triangle"]
            assert b.area[w[w >= 0]].all(), (name, f)
        if not hasattr(b.sd, "planted"):
            continue
        # (a scaled or translated copy rounds the corners again: the collinear triangles gain a sliver of area there, the ones with a
        # repeated corner never do)
        assert (~b.area[b.sd.planted["no_area"]]).sum() >= 4 and b.area[b.sd.planted["slivers"]].all(), name
        if name == "soup":
            assert (~b.area[b.sd.planted["no_area"]]).all() and b.area[b.sd.planted["tiny"]].all()
        w = b.brute[0]["triangle"]
        for lower, upper in b.sd.planted["ties"]:
            assert lower < upper and b.V[lower].tobytes() == b.V[upper].tobytes()
            assert (w == lower).sum() >= 40 and (w == upper).sum() == 0, (name, lower, upper, int((w == lower).sum()), int((w == upper).sum()))
        hub = (b.V[b.sd.planted["fan"]].reshape(-1, 3, 3) == b.sd.fan_hub).all(axis=2).any(axis=1)
        assert hub.all() and np.isin(w, b.sd.planted["fan"]).sum() >= 8, name


def test_far_rays_aimed_just_inside_corners_and_outlines_mostly_hit(batches):
    for name, b in batches.items():
        for R in rh.FAR_R:
            k = f"far {R:g}"
            m = b.kinds == k
            r = b.rays[m]
            hit = b.brute[0]["triangle"][m] >= 0
            full = r[:, 7] > 1.0e38                     # (every eighth far bound ends short of the target on purpose)
            for what in ("vertex", "outline"):
                sel = (b.far_target[R] == what) & full
                share = float(hit[sel].mean())
                say(f"{name:14s} {k:10s} {what:8s} {int(sel.sum())} rays, hit share {share:.3f}")
                if (name, k) in BEYOND_FP32:
                    continue
                assert share >= 0.6, (name, k, what, share)


def test_a_direction_scaled_by_a_power_of_two_keeps_its_winner(batches):
    for name, b in batches.items():
        base = b.osc.closest_brute(b.scaled_base, 0)
        assert (base["triangle"] >= 0).mean() > 0.2
        for e in rh.SCALES:
            got = b.brute[0][b.kinds == f"scaled d 2^{e}"]
            same = got["triangle"] == base["triangle"]
            say(f"{name:14s} scaled d 2^{e}: {int(same.sum())} of {len(same)} winners kept")
            if abs(e) > 64:
                # the device refuses these (include/evplp.h).  The triangle test itself is no longer exact under the scaling: n . d of
                # the 1e-3 soup's small triangles is subnormal at 2^-100, q overflows on the 1e3 soup at 2^100
                continue
            assert same.all(), (name, e, np.nonzero(~same)[0][:8])
            hit = base["triangle"] >= 0
            assert got["beta"][hit].tobytes() == base["beta"][hit].tobytes() and got["gamma"][hit].tobytes() == base["gamma"][hit].tobytes()
            assert np.array_equal(got["t"][hit], np.ldexp(base["t"][hit], -e)), (name, e)


def test_the_c_brute_force_equals_the_python_one_on_64_rays(batches):
    for name in ("soup", "room"):
        b = batches[name]
        rng = np.random.RandomState(3)
        pick = np.sort(rng.choice(np.nonzero(b.valid)[0], 64, replace=False))
        rays = b.rays[pick]
        table = brute_table(b.osc, b.V, rays)
        for f in (0, 1, 2):
            want = brute_closest(table, rays, b.light, f)
            got = b.osc.closest_brute(rays, f)
            assert got.tobytes() == want.tobytes(), (name, f, np.nonzero(got != want)[0][:8])
            assert got.tobytes() == b.brute[f][pick].tobytes()
        occ = b.osc.occluded_brute(rays)
        assert np.array_equal(occ == 1, (table[0] & (table[1] < rays[:, 7:8])).any(axis=1))
