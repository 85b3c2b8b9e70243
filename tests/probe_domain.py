"""Inputs and float64 references of the probe gather (include/evplp.h "probe gather") over the material domain of shading_domain.py and on
hostile (record, probe) pairs.  numpy only; the oracle serves for the visibility of the shadow rays.  Shared by test_probe_host.py,
test_probe_domain_host.py (evplp_probe_pair, no GPU), test_gpu_probe.py and test_gpu_probe_domain.py (probe_gather_kernel).

The material domain: scene shading_domain.floor_scene(), records shading_domain.make_vpls() (37 classes in 64 slots, 32 paths x 2, so the
division by the path count is exact), and per record the 369 probes of positions_for().

The hostile pairs have a scene of their own (hostile_scene: the floor at z = -5, the light at z = 90, the origin in free space), records
at (0, 0, 0) (hostile_records) and probes (hostile_probes) that visit what include/evplp.h says about dist2 = (v.x v.x + v.y v.y) + v.z v.z
in float32: a pair whose dist2 is not a normal finite number casts no ray, adds no term and is not counted.  The families:
  near_walked   2^-20 .. 2^-62 from the record along its normal and obliquely: inside min_distance (the clamp), finite, lit
  near_edge     axis-aligned 2^-63 (dist2 = 2^-126 exactly: walked), 2^-63 (1 - 2^-23), 2^-64, 2^-65 (skipped), and (d, d, d) with
                d = fl(2^-63.5): three subnormal squares whose sum is normal (walked only if the squares are not flushed)
  near_below    2^-70, 2^-100, 2^-126, a subnormal, and the record's own position: skipped
  far_walked    1e3, 1e6, 2^40, 2^63 along +-x and +-y (5 units above the floor: nothing near the rays)
  far_edge      2^64 (1 - 2^-24) (dist2 finite: walked), 2^64, 2^100, 3e38, (3e38, 3e38, 3e38) (dist2 = inf: skipped)
  invalid       a NaN, +inf, -inf coordinate: c = 0, lit = -1
  lobe_cut      e = 1000, the lobe's cosine 1e-5 and 1e-7 either side of the cut 1e-6 (the latter undecided: compared with nothing), and
                5e-6 above it, where the same lobe with e = 0 tells the cut 1e-6 from 1e-5
  ordinary      a few points of the room, which the placement tests fill waves with
The bound is the project's: shading_domain.bar(term, kappa, lam, K, hw_pow) per pair, K = K_ORACLE_PROBE with hw_pow = False for the host
twin and twice that with hw_pow = True for the kernel, plus lit 2^-24 sum |term| where several pairs are summed in float32."""
import math

import numpy as np

import oracle_api as oa
import probe_restate as pr
import shading_domain as sd

F = np.float32
MIN_DISTANCE = 0.05
NPATHS, P = sd.NPATHS, sd.P
# The smallest K that holds, measured 2026-10-20 with `pytest -s -m "not gpu" tests/test_probe_host.py` (the pair test prints the worst
# error / (2^-24 kappa |f64|) it meets): 5.46 over 37 records x 367 positions (11 311 facing pairs, none of them undecided), rounded up.
K_ORACLE_PROBE = 6
K_GPU_PROBE = 2 * K_ORACLE_PROBE
TMIN, TMAX = F(0.0001), F(1.0) - F(0.0001)
SLICE_PATHS, SLICE_SLOTS = 288, 576                     # two full slices of EVPLP_PROBE_SLICE_SLOTS and 64 slots of a third
SLICE_PLACES = (0, 255, 256, 511, 512, 575)


def say(*a):
    print("[probe]", *a, flush=True)


def positions_for(rec):
    """(positions [m, 3] float32, kind per position) for one record"""
    pos = rec["pos"].astype(np.float64); n = rec["normal"].astype(np.float64)
    gx, gy = np.meshgrid(np.linspace(-11.0, 11.0, 15), np.linspace(-7.0, 7.0, 12))
    grid = [np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, z)], -1) for z in (0.0, 0.35)]
    parts, kinds = [], []

    def add(kind, p):
        p = np.asarray(p, np.float64).reshape(-1, 3); parts.append(p); kinds.extend([kind] * len(p))
    add("grid", np.concatenate(grid))
    add("behind", [pos - 0.7 * n, pos - 3.0 * n + [0.4, -0.2, 0.0]])
    add("inside_min_distance", [pos + 0.3 * MIN_DISTANCE * n, pos + 0.9 * MIN_DISTANCE * (n + [0.3, 0.1, 0.0]) / np.linalg.norm(n + [0.3, 0.1, 0.0])])
    add("at_vpl", [pos])
    r = sd._mirror(rec["flux_dir"].astype(np.float64), n)                      # the lobe's axis: reflect(-fdir, n)
    r = r / np.linalg.norm(r)
    add("on_lobe", [pos + 1.5 * r, pos + 0.4 * r])
    t = np.cross(r, [0.3, 0.5, 0.81]); t /= np.linalg.norm(t)
    add("lobe_flank", [pos + 1.5 * (r + 0.05 * t), pos + 1.5 * (r + 0.5 * t)])
    return np.concatenate(parts).astype(F), np.array(kinds, object)


def oracle_occluded_tree(osc, rays):
    out = np.zeros(rays.shape[0], np.uint8)
    for i, r in enumerate(rays):
        o, d = np.ascontiguousarray(r[0:3]), np.ascontiguousarray(r[4:7])
        out[i] = osc.lib.evo_occluded(osc.h, oa.ptr(o), oa.ptr(d), float(r[3]), float(r[7]))
    return out


class Reference:
    """every (usable slot, probe) pair once: the float32 cosine test and dist2 test, the shadow rays, the oracle's visibility, the float64
    terms.  per_path: the records per light path (a call reads the slots < paths * per_path); K, hw_pow: the bar's."""

    def __init__(self, osc, records, probes, min_distance=MIN_DISTANCE, tree=True, *, per_path, K=K_GPU_PROBE, hw_pow=True):
        self.records, self.probes, self.per_path = records, probes, per_path
        n = probes.shape[0]
        self.slots = np.nonzero(records["flags"] & 1)[0]
        K_ = len(self.slots)
        self.facing = np.zeros((K_, n), bool); self.walked = np.zeros((K_, n), bool)
        self.term = np.zeros((K_, n, 9, 3)); self.bar = np.zeros((K_, n, 9, 3)); self.decided = np.ones((K_, n), bool)
        rays, where = [], []
        for j, k in enumerate(self.slots):
            cos32, v12 = pr.facing_f32(records[k], probes)
            self.walked[j] = pr.walked_f32(records[k], probes)
            f32 = cos32 & self.walked[j]                                          # the pair casts a shadow ray
            term, kappa, lam, decided, f64 = pr.pair_f64(records[k], probes, min_distance)
            self.facing[j] = f32
            self.decided[j] = decided & (f32 == f64)
            self.term[j] = term
            self.bar[j] = sd.bar(term, kappa, lam, K, hw_pow)
            idx = np.nonzero(f32)[0]
            r = np.zeros((len(idx), 8), F)
            r[:, 0:3] = records["pos"][k]; r[:, 3] = TMIN; r[:, 4:7] = -v12[idx]; r[:, 7] = TMAX
            rays.append(r); where.append(np.stack([np.full(len(idx), j), idx], -1))
        self.rays = np.concatenate(rays); self.where = np.concatenate(where)
        self.set_visibility(osc, tree)

    def set_visibility(self, osc, tree=True):
        """the oracle scene's answers for the shadow rays (again after the scene has moved)"""
        brute = osc.occluded_brute(self.rays)
        self.aside_rays = (oracle_occluded_tree(osc, self.rays) != brute) if tree else np.zeros(len(brute), bool)
        self.occluded_rays = brute
        K_, n = self.facing.shape
        self.lit = np.zeros((K_, n), bool); self.aside = np.zeros((K_, n), bool)
        self.lit[self.where[:, 0], self.where[:, 1]] = brute == 0
        self.aside[self.where[:, 0], self.where[:, 1]] = self.aside_rays

    def expect(self, paths, keep=None):
        """(c [n, 9, 3] float64, bar [n, 9, 3], lit [n], undecided per probe [n]) of the slots < paths * per_path, of those only keep[slot]"""
        use = self.slots < paths * self.per_path
        if keep is not None:
            use &= keep[self.slots]
        lit = self.lit & use[:, None]
        m = lit[:, :, None, None]
        und = lit & ~self.decided
        mag = np.abs(self.term)
        total = np.where(m, self.term, 0.0).sum(0)
        count = lit.sum(0)
        bar = np.where(m & self.decided[:, :, None, None], self.bar, 0.0).sum(0) + np.where(und[:, :, None, None], mag + self.bar, 0.0).sum(0)
        bar = bar + count[:, None, None] * 2.0 ** -24 * np.where(m, mag, 0.0).sum(0)
        return total / paths, bar / paths, count, und.sum(0)


def check_values(got, ref, paths, what, keep=None):
    c, bar, lit, und = ref.expect(paths, keep)
    skip = (ref.aside & (ref.slots < paths * ref.per_path)[:, None]).any(0)
    ok = ~skip
    assert np.array_equal(got["lit"][ok], lit[ok].astype(F)), (what, np.nonzero(got["lit"] != lit)[0][:8], got["lit"][:8], lit[:8])
    err = np.abs(got["c"].astype(np.float64) - c)
    bad = np.argwhere((err > bar) & ok[:, None, None])
    worst = float((err / np.maximum(bar, 1e-300))[ok].max()) if ok.any() else 0.0
    say(f"{what}: {int(lit.sum())} lit pairs, worst error / bar = {worst:.3f}, undecided {int(und.sum())} (worst probe {int(und.max()) if len(und) else 0})")
    assert bad.size == 0, (what, bad[:4].tolist(), got["c"][tuple(bad[0])], c[tuple(bad[0])], bar[tuple(bad[0])])
    return lit


def check_single(c, lit, ref, mask, what, labels=None):
    """one usable record (ref has one slot): c [n, 9, 3], the coefficients times the path count (exact: a power of two), against the pair's
    own term under the pair's own bar -- no summation, so nothing is granted for one.  mask [n]: the pairs expected to carry their term
    (ref.lit[0] for the kernel, ref.facing[0] for the host twin, whose visibility is 1); every other entry must be exactly 0.  lit (or
    None): the kernel's count, which must equal mask.  A pair the oracle's two walks disagree on is set aside, an undecided one is
    compared with nothing (but must be finite).  Returns the worst error / bar of the decided pairs."""
    assert len(ref.slots) == 1
    c = np.asarray(c, np.float64)
    ok = ~ref.aside[0]
    assert np.isfinite(c).all(), (what, np.argwhere(~np.isfinite(c))[:4].tolist())
    if lit is not None:
        wrong = np.nonzero((np.asarray(lit) != mask.astype(F)) & ok)[0]
        assert wrong.size == 0, (what, "lit", wrong[:8].tolist(), None if labels is None else [labels[i] for i in wrong[:8]], np.asarray(lit)[wrong[:8]])
    off = ok & ~mask
    assert (c[off] == 0.0).all(), (what, "a term without a lit pair", np.nonzero(off & (c != 0).any(axis=(1, 2)))[0][:8].tolist())
    on = ok & mask & ref.decided[0]
    err = np.abs(c - ref.term[0])
    ratio = np.where(on[:, None, None], err / ref.bar[0], 0.0)
    bad = np.argwhere(ratio > 1.0)
    assert bad.size == 0, (what, bad[:4].tolist(), None if labels is None else labels[bad[0, 0]], ref.probes[bad[0, 0]], c[tuple(bad[0])],
                           ref.term[0][tuple(bad[0])], ref.bar[0][tuple(bad[0])])
    return float(ratio.max()) if ratio.size else 0.0


# ------------------------------------------------------------------------------------------------------------------ the material domain
def domain_records():
    recs, names = sd.make_vpls()
    return recs, names


def grid_probes(rec):
    X, kinds = positions_for(rec)
    return X[kinds == "grid"]                         # (the same 360 points under every record)


# ------------------------------------------------------------------------------------------------------------------ hostile pairs
def hostile_scene():
    """the floor quad at z = -5 and the light quad at z = 90: the origin, where the records sit, lies in free space"""
    import scenes
    s = scenes.SceneData()
    s.aspect = sd.W / sd.H
    floor = s.add_material((0.5, 0.5, 0.5))
    s.add_quad([-12.0, -8.0, -5.0], [24.0, 0.0, 0.0], [0.0, 16.0, 0.0], floor)
    lm = s.add_material((0, 0, 0))
    s.light_mesh = s.add_quad([-0.5, -0.5, 90.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], lm)
    s.light_intensity = [1.0, 1.0, 1.0, 0.0]
    s.cam_origin = list(sd.CAMERA); s.cam_lookat = [0.0, 0.0, 0.0]; s.cam_up = [0.0, 1.0, 0.0]
    s.fovy = sd.FOVY
    s.triangle_soup()
    return s


AXES = {"+z": (0.0, 0.0, 1.0), "+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0), "+y": (0.0, 1.0, 0.0), "-y": (0.0, -1.0, 0.0)}
OBLIQUE = (0.6, 0.0, 0.8)
FLUXES = (1e-30, 1e-12, 1e12, 1e25)
CUT_AXIS, CUT_FLANK = np.array([0.8, 0.0, 0.6]), np.array([-0.6, 0.0, 0.8])     # the e = 1000 lobe's axis and a unit vector across it, both facing +z


def hostile_records():
    """(records [64], name per usable slot, usable slots): every record at (0, 0, 0), usable ones spread over the slots with unusable ones
    (flags 0, flux 1e30) before, between and behind them"""
    RS, RD = (0.3, 0.2, 0.4), (0.5, 0.6, 0.4)
    out = []

    def add(name, n, axis=None, e=0.0, flux=(1.0, 0.8, 1.2)):
        n = np.asarray(n, np.float64)
        fdir = n if axis is None else sd._mirror(sd._unit(axis), n)         # reflect(-fdir, n) = axis
        out.append((name, (0.0, 0.0, 0.0), n, fdir, flux, RD, (0.0, 0.0, 0.0) if axis is None else RS, e, 1.0 if axis is None else 0.3))
    for d, n in AXES.items():
        add("lambert_" + d, n)
        add("glossy_" + d, n, axis=n, e=20.0)
    add("glossy_oblique", AXES["+z"], axis=OBLIQUE, e=20.0)
    for f in FLUXES:
        add(f"lambert_flux{f:g}", AXES["+z"], flux=(f, 0.5 * f, 2.0 * f))
        add(f"glossy_flux{f:g}", AXES["+z"], axis=AXES["+z"], e=20.0, flux=(f, 0.5 * f, 2.0 * f))
    add("lobe_cut_e1000", AXES["+z"], axis=CUT_AXIS, e=1000.0)
    add("lobe_cut_e0", AXES["+z"], axis=CUT_AXIS, e=0.0)       # d^0 = 1: whether the lobe is on at 6e-6 shows in the value (1e-5 is the GLSL cut)
    rec = np.zeros(NPATHS * P, dtype=oa.RECORD_DTYPE)
    rec["flux"] = sd.BIG
    slots = [2 + 3 * i for i in range(len(out))]              # 2, 5, .. 59: slots 0, 1, 60 .. 63 and two of every three between stay unusable
    assert slots[-1] < len(rec) - 1
    for k, (name, *fields) in zip(slots, out):
        sd._fill(rec, k, *fields, flags=1)
    return rec, [o[0] for o in out], slots


def hostile_probes():
    """(positions [m, 3] float32, family per position, label per position)"""
    pts, fam, lab = [], [], []

    def add(family, label, p):
        pts.append(np.asarray(p, F)); fam.append(family); lab.append(label)
    z, ob = np.array(AXES["+z"], F), np.array(OBLIQUE, F)
    for k in (20, 40, 60, 62):
        add("near_walked", f"2^-{k} n", F(2.0 ** -k) * z)
        add("near_walked", f"2^-{k} oblique", F(2.0 ** -k) * ob)
    add("near_edge", "2^-63", F(2.0 ** -63) * z)
    add("near_edge", "2^-63 (1 - 2^-23)", F(2.0 ** -63 * (1.0 - 2.0 ** -23)) * z)
    add("near_edge", "2^-64", F(2.0 ** -64) * z)
    add("near_edge", "2^-65", F(2.0 ** -65) * z)
    add("near_edge", "2^-63.5 (1, 1, 1)", np.full(3, F(2.0 ** -63.5)))
    for k in (70, 100, 126):
        add("near_below", f"2^-{k}", F(2.0 ** -k) * z)
    add("near_below", "subnormal", F(2.0 ** -140) * z)
    add("near_below", "at the record", np.zeros(3, F))
    for name in ("+x", "-x", "+y", "-y"):
        for d, dl in ((1e3, "1e3"), (1e6, "1e6"), (2.0 ** 40, "2^40"), (2.0 ** 63, "2^63")):
            add("far_walked", f"{dl} {name}", F(d) * np.array(AXES[name], F))
    x = np.array(AXES["+x"], F)
    add("far_edge", "2^64 (1 - 2^-24)", F(2.0 ** 64 * (1.0 - 2.0 ** -24)) * x)
    add("far_edge", "2^64", F(2.0 ** 64) * x)
    add("far_edge", "2^100", F(2.0 ** 100) * x)
    add("far_edge", "3e38", F(3e38) * x)
    add("far_edge", "3e38 (1, 1, 1)", np.full(3, F(3e38)))
    add("invalid", "nan", [np.nan, 0.0, 1.0])
    add("invalid", "+inf", [1.0, np.inf, 0.0])
    add("invalid", "-inf", [0.0, 1.0, -np.inf])
    for off, ol in ((1e-5, "+1e-5"), (-1e-5, "-1e-5"), (1e-7, "+1e-7"), (-1e-7, "-1e-7"), (5e-6, "+5e-6")):
        d = sd.CUT_CUDA + off
        add("lobe_cut", f"cut {ol}", 1.5 * (CUT_FLANK * math.sqrt(1.0 - d * d) + CUT_AXIS * d))
    for p in ((0.3, 0.2, 1.5), (-1.0, 0.5, 0.7), (2.0, -1.0, 3.0), (0.02, 0.0, 0.03), (-2.5, -1.5, 0.4), (1.0, 2.0, -0.5)):
        add("ordinary", str(p), p)
    return np.stack(pts).astype(F), np.array(fam, object), np.array(lab, object)


def valid_probes(x):
    return np.isfinite(x).all(axis=1)


def hostile_reference(osc, K, hw_pow):
    """(records, names, slots, probes, family, label, {slot: Reference of that record alone on the valid probes})"""
    rec, names, slots = hostile_records()
    X, fam, lab = hostile_probes()
    ok = valid_probes(X)
    refs = {k: Reference(osc, sd.only_slot(rec, k, 1), X[ok], per_path=P, K=K, hw_pow=hw_pow) for k in slots}
    return rec, names, slots, X, fam, lab, refs


def expected_walk(names, fam, lab):
    """what the families are built to visit, stated from their construction and not through walked_f32: {(record name, probe index):
    True the pair casts a ray, False it is skipped} for the records that face the family (normal +z for the near ones, +x for the far
    edge, the probe's own axis for far_walked)"""
    want = {}
    for i, (f, l) in enumerate(zip(fam, lab)):
        for name in names:
            axis = name.split("_")[-1]
            if axis == "+z" and f in ("near_walked", "near_edge", "near_below"):
                want[name, i] = f == "near_walked" or l in ("2^-63", "2^-63.5 (1, 1, 1)")
            elif f == "far_walked" and axis == l.split()[-1]:
                want[name, i] = True
            elif f == "far_edge" and axis == "+x":
                want[name, i] = l == "2^64 (1 - 2^-24)"
    return want


def filler_variants(rec):
    """the records with every float of every unusable slot set to 0, NaN, +inf and 1e30 in turn (flags stay 0): {name: records}"""
    out = {}
    dead = (rec["flags"] & 1) == 0
    for name, v in (("zero", 0.0), ("nan", np.nan), ("inf", np.inf), ("1e30", 1e30)):
        r = rec.copy()
        words = r.view(F).reshape(len(r), -1)
        words[dead] = F(v)
        r["flags"][dead] = 0
        assert np.array_equal((r["flags"] & 1) == 0, dead) and r[~dead].tobytes() == rec[~dead].tobytes()
        out[name] = r
    return out


def wave_batch(X, fam):
    """the hostile, invalid and ordinary probes in one batch of 2 x 64 + 1: hostile ones at lanes 0, 31 and 63 of both full waves and alone in
    the ragged last wave, the rest of the hostile and invalid ones spread between, ordinary ones everywhere else.  Returns the index
    into X per batch entry."""
    ordinary = np.nonzero(fam == "ordinary")[0]
    special = [i for i in range(len(X)) if fam[i] != "ordinary"]
    src = ordinary[np.arange(129) % len(ordinary)]
    pick = lambda f, j: [i for i in special if fam[i] == f][j]                   # noqa: E731
    corner = {0: pick("near_below", 4), 31: pick("far_edge", 3), 63: pick("near_edge", 1), 64: pick("near_walked", 7), 95: pick("invalid", 0),
              127: pick("far_walked", 15), 128: pick("near_edge", 0)}
    for at, i in corner.items():
        src[at] = i
    rest = [i for i in special if i not in corner.values()]
    free = [at for at in range(1, 127, 2) if at not in corner]
    assert len(rest) <= len(free)
    for at, i in zip(free, rest):
        src[at] = i
    assert set(special) <= set(src.tolist()) and all(fam[src[at]] != "ordinary" for at in corner)
    return src


def slice_records(osc_records_dtype, record, place):
    """SLICE_SLOTS slots, every float a NaN and flags 0, `record` alone usable at slot `place`"""
    r = np.zeros(SLICE_SLOTS, dtype=osc_records_dtype)
    r.view(F).reshape(SLICE_SLOTS, -1)[:] = np.nan
    r["flags"] = 0
    r[place] = record
    return r


def slice_probes():
    """70 probes: the hostile ones and ordinary points of the room above the record"""
    X, fam, lab = hostile_probes()
    rng = np.random.RandomState(20264)
    more = np.stack([rng.uniform(-3.0, 3.0, 70 - len(X)), rng.uniform(-3.0, 3.0, 70 - len(X)), rng.uniform(0.2, 4.0, 70 - len(X))], -1).astype(F)
    return np.concatenate([X, more])
