"""Hostile sums for the statistics kernels (kernels_stats.hip: the noise fold, shard pooling, evplp_noise_estimate, evplp_noise_variance,
evplp_adaptive_retire, evplp_adaptive_tile_noise, evplp_frame_error) and their two references (numpy only, no GPU).

The other statistics tests see natural renders, or rng.random() planes in [0, 1), and restate the library's own expression
(Q - S^2 / K) / (B - 1).  Here the caller chooses every sum: the accumulators are uploaded before every fold, so each pixel's batch increments
are what the case says, to the bit.  upload_case() does that on a context; host_composite() is resolve_kernel's expression in numpy, so
that tests/test_stats_hostile_host.py can prove what the cases are and that the bars are reachable without a device.

Planes.  A frame is W x H image pixels in `rows` = 8 ceil(H / 8) plane rows, y = 0 at the bottom.  EVERY ROW PAST H holds 1e30 in even
columns and NaN in odd columns, in every uploaded plane (both accumulators, the light plane): only the `y < H` tests of the kernels keep
them out.  The photon accumulator is zero inside the image, so c = vpl + photon is the uploaded VPL sum, exactly.

Families (make_case; states[0] is where tracking starts, one fold of schedule[j - 1] iterations closes at states[j]):
  decades        the signal times 10^(-12 .. 12) along x, noise in proportion, folds of unequal size (1, 3, 2, 2); variant 1: 10^(-6 .. 6) and
                 folds of (1, 2^20, 3, 2^10) iterations
  late_start     tracking starts on sums of about 2^24 times the per-iteration value and the sums grow in fp32 as an accumulator's do: the
                 increments land on the ulp grid, and in every fourth column (sums of 2^26 times it, increments a sixteenth) they vanish:
                 D = 0 in every fold and v is exactly 0
  inexact_S      c_start of magnitude 2^-6 (negative in odd columns: a caller can upload that) under sums of 2^25 and more, 30 binades
                 apart: the fp32 c_prev - c_start rounds, and so does the first D.  The batch means agree to about 1e-6, so Q - S^2 / K
                 cancels to roundings and the clamp decides
  zero_variance  even columns: increments k_j d with d a power of two on sums that are multiples of d: Q - S^2 / K is exactly 0.  Odd
                 columns: the same with d = 0.1 times the signal, summed in fp32: v is a rounding of either sign, reads 0 or stays in the bar
  emitters       light.x by column, x % 6: 0, 1e-30 (times a light_scale of 1e-20 it underflows to 0), -0.5, NaN, 2, and 0 under light.y = 3;
                 estimated at light scales 1, 1e-20, 0 and -1, each with mask_emitter 0 and 1.  A NaN light makes the composite NaN: broken
                 (the case's mask keeps those columns out, so the third figure stays finite)
  nonfinite      single pixels (marks): +Inf from the first fold on in the one tile with exactly one broken pixel; a tile whose every pixel is
                 broken (+Inf, -Inf, NaN by turns, from the first fold, from a middle fold, only in the last, in each channel by turns); a
                 NaN in the partial tile column; a -Inf of the last fold alone in the partial tile row; an Inf that the next upload replaces
                 with a finite sum (S and the composite are finite, Q and v are +Inf: broken by v alone); sums of 1e20 whose variance exceeds
                 fp32 (v is finite in fp64: sound, and evplp_noise_variance reads Inf); a composite of 2^120 with a variance of exactly 0
                 (sound -- until a scale of 1e20 takes its composite to Inf)
  masks          nonfinite's sums under three masks: keep nothing (the third figure is 0), keep only broken pixels (it is NaN), keep sound
                 pixels by a single non-zero byte (it is finite)
Every case is estimated at the scales 1 / K, 0, -1 / K, 1e-20 and 1e20 (emitters: at 1 / K and its four light scales).

The rule (include/evplp.h, "non-finite sums").  A pixel is BROKEN when its den is not finite, or -- unless mask_emitter hides it -- any of
its three v = (Q - S^2 / K) / (B - 1) is not.  An image figure that a broken pixel enters is NaN; a tile figure is the mean over the tile's
sound in-image pixels, 0 when it has none; evplp_noise_variance keeps its bytes (a NaN v reads 0, an infinite one Inf -- times a scale of
exactly 0 that is NaN).

References.  restate() is the numpy restatement the statistics tests share (test_gpu_noise.numpy_variance / numpy_figures,
test_gpu_adaptive.rel_of / tile_means), with the rule: the variance image bit for bit, figures to 1e-12.  statement64() shares no line with
it and never forms Q - S^2 / K: per pixel and channel it takes the differences D_j = c_j - c_{j-1} of the fp32 sums in float64, the batch
means m_j = D_j / k_j, the pooled mean m = sum D_j / K and s2 = sum k_j (m_j - m)^2 / (B - 1) in two passes; the variance is scale^2 K s2.
Its broken set comes from the sums themselves: a non-finite sum at any fold boundary (every such sequence makes Q or S^2 / K non-finite or
their difference NaN), or a difference beyond fp32 (the library's D and S are fp32), or a non-finite composite.

The bar against statement64 is derived, not measured.  The library's D_j and S are fp32 subtractions, each within 2^-24 relative of the exact
difference, so D_j^2 and S^2 are within 2^-23 (to first order), and per channel |v_lib - v_ref| <= 2^-23 (Q_ref + S_ref^2 / K) / (B - 1).
The clamp only moves v_lib toward v_ref >= 0.  The bar is twice that, times s2K: the factor 2 covers the float64 roundings of both sides and
the second-order terms.  A figure's bar is the sum of its pixels' bars over den, plus 1e-12 relative (the summation orders).  No pixel is
set aside."""
from types import SimpleNamespace

import numpy as np

from test_gpu_adaptive import rel_of, tile_means
from test_gpu_noise import numpy_figures, numpy_variance

f32, f64 = np.float32, np.float64
FLT_MAX = float(np.finfo(f32).max)
FRAMES = ((37, 21), (259, 13), (5, 3))
FAMILIES = ("decades", "late_start", "inexact_S", "zero_variance", "emitters", "nonfinite", "masks")
SCHEDULE = (1, 3, 2, 2)
BIG_SCHEDULE = (1, 1 << 20, 3, 1 << 10)
# (family, W, H, variant)
CASES = [(fam, 37, 21, 0) for fam in FAMILIES[:6]] + [("decades", 37, 21, 1)] + [("masks", 37, 21, v) for v in (0, 1, 2)] + \
        [(fam, 259, 13, 0) for fam in ("decades", "inexact_S", "emitters", "nonfinite")] + [("masks", 259, 13, 2)] + \
        [(fam, 5, 3, 0) for fam in ("zero_variance", "nonfinite", "late_start")]


def case_id(case):
    return "%s-%dx%d-%d" % tuple(case)


def plane_rows(H):
    return (H + 7) // 8 * 8


def tiles_of(W, H):
    return (W + 7) // 8, (H + 7) // 8


def _hostile_rows(p, H):
    p[H:, 0::2] = f32(1e30); p[H:, 1::2] = f32(np.nan)
    return p


def _plane(a, H, W):
    out = np.zeros((plane_rows(H), W, 4), f32)
    out[:H, :, :3] = a
    return _hostile_rows(out, H)


def _accumulate(c0, incs):
    """the states of an fp32 accumulator that starts at c0 and takes the increments one by one"""
    states = [np.asarray(c0, f32)]
    for d in incs:
        states.append((states[-1] + np.asarray(d, f32)).astype(f32))
    return states


def _poison(states, y, x, ch, value, first, last=None):
    for j in range(first, (len(states) - 1 if last is None else last) + 1):
        states[j][y, x, ch] = value


def nonfinite_marks(W, H, B):
    """where the nonfinite family puts what (pixels as (y, x), tiles as (ty, tx)); a frame too small for a placement leaves it out"""
    TX, TY = tiles_of(W, H)
    m = dict(one=(min(3, H - 1), min(2, W - 1)), all_tile=None, col=None, row=None, replaced=None)
    if TX == 1:
        m.update(variance=(0, 0), overflow=(1, W - 1))
        return m
    m["all_tile"] = (min(1, TY - 1), 1)
    m["col"] = (min(5, H - 1), W - 2)                       # tile (0, TX - 1): the partial tile column
    m["row"] = (H - 2, 26)                                  # tile (TY - 1, 3): the partial tile row
    m["replaced"] = (2, 20)                                 # tile (0, 2)
    y = min(10, H - 3)
    m.update(variance=(y, 20), overflow=(y, 33))            # tiles (1, 2) and (1, 4)
    return m


def make_case(family, W, H, variant=0):
    assert family in FAMILIES
    rng = np.random.default_rng([FAMILIES.index(family), W, H, variant, 20261021])
    jj, ii = np.meshgrid(np.arange(H, dtype=f64), np.arange(W, dtype=f64), indexing="ij")
    xi = ii.astype(np.int64)
    base = (1.0 + 0.5 * np.sin(0.3 * ii) + 0.3 * np.cos(0.4 * jj))[..., None] * np.array([1.0, 0.8, 0.6])
    schedule = SCHEDULE
    light = np.zeros((H, W, 3), f32)
    mask = None
    marks = {}
    calls = None

    def noisy(signal, sched, sigma=0.3):
        return [k * signal * np.clip(1.0 + sigma / np.sqrt(k) * rng.standard_normal((H, W, 3)), 0.0, 1.9) for k in sched]

    if family == "decades":
        span = 12.0 if variant == 0 else 6.0
        schedule = SCHEDULE if variant == 0 else BIG_SCHEDULE
        signal = base * 10.0 ** (np.linspace(-span, span, W) if W > 1 else np.zeros(1))[None, :, None]
        states = _accumulate(np.zeros((H, W, 3)), noisy(signal, schedule))
    elif family == "late_start":
        vanish = (xi % 4 == 3)
        start = np.where(vanish[..., None], 2.0 ** 26, 2.0 ** 24) * base * rng.uniform(0.5, 2.0, (H, W, 3))
        per_it = np.where(vanish[..., None], base / 16.0, base)
        states = _accumulate(start, noisy(per_it, schedule))
        marks["vanish"] = vanish
    elif family == "inexact_S":
        c0 = rng.uniform(2.0 ** -6, 2.0 ** -5, (H, W, 3)) * np.where(xi % 2 == 1, -1.0, 1.0)[..., None]
        m = 2.0 ** 25 * rng.uniform(1.0, 2.0, (H, W, 3))
        states = _accumulate(c0, [k * m * (1.0 + 2.0 ** -20 * rng.standard_normal((H, W, 3))) for k in schedule])
    elif family == "zero_variance":
        exact = (xi % 2 == 0)
        d2 = 2.0 ** rng.integers(-3, 4, (H, W, 3)).astype(f64)
        d = np.where(exact[..., None], d2, (f32(0.1) * base.astype(f32)).astype(f64))
        c0 = np.where(exact[..., None], d2 * rng.integers(0, 100, (H, W, 3)), 0.0)
        states = _accumulate(c0, [(f32(k) * d.astype(f32)).astype(f32) for k in schedule])
        marks["exact"] = exact
    elif family == "emitters":
        states = _accumulate(np.zeros((H, W, 3)), noisy(base, schedule))
        kind = xi % 6
        lx = np.select([kind == 1, kind == 2, kind == 3, kind == 4], [1e-30, -0.5, np.nan, 2.0], 0.0)
        light[..., 0] = lx; light[..., 1] = np.where(kind == 5, 3.0, 0.5 * np.nan_to_num(lx)); light[..., 2] = 0.25 * np.nan_to_num(lx)
        marks["kind"] = kind
        mask = np.zeros((H, W, 3), np.uint8)                # the mask keeps the NaN lights out: the third figure stays finite
        mask[::-1][kind != 3] = 255
        s = 1.0 / sum(schedule)
        calls = [(s, ls, me) for ls in (1.0, 1e-20, 0.0, -1.0) for me in (False, True)]
    else:                                                   # nonfinite, masks
        states = _accumulate(np.zeros((H, W, 3)), noisy(base, schedule))
        B = len(schedule)
        m = nonfinite_marks(W, H, B)
        cum = np.concatenate([[0], np.cumsum(schedule)])
        _poison(states, *m["one"], 0, np.inf, 1)
        if m["all_tile"] is not None:
            ty, tx = m["all_tile"]
            n = 0
            for y in range(8 * ty, min(8 * ty + 8, H)):
                for x in range(8 * tx, min(8 * tx + 8, W)):
                    value, first = (np.inf, -np.inf, np.nan)[n % 3], (1, 2, B)[(n // 3) % 3]
                    _poison(states, y, x, (n // 9) % 3, value, first)
                    n += 1
            _poison(states, *m["col"], 1, np.nan, 1)
            _poison(states, *m["row"], 2, -np.inf, B)
            _poison(states, *m["replaced"], 0, np.inf, 2, 2)
        y, x = m["variance"]
        for j in range(1, B + 1):
            states[j][y, x] = states[j - 1][y, x] + f32(schedule[j - 1]) * f32(1e20 if j % 2 else 3e20)
        y, x = m["overflow"]
        for j in range(B + 1):
            states[j][y, x] = f32(cum[j]) * f32(2.0 ** 120)
        marks.update(m)
        if family == "masks":
            broken = statement_broken(states, np.zeros((H, W), bool)) if variant == 1 else None
            mask = np.zeros((H, W, 3), np.uint8)                        # top-down, as evplp_noise_track takes it
            if variant == 1:
                mask[::-1][broken] = 255
            elif variant == 2:
                keep = (rng.random((H, W)) < 0.4) & ~statement_broken(states, np.zeros((H, W), bool))
                keep[H - 1, :] = False; keep[0, 0] = True                # (no symmetry between top and bottom)
                mask[::-1][keep, 1] = 1
    K = sum(schedule)
    if calls is None:
        calls = [(s, 1.0, False) for s in (1.0 / K, 0.0, -1.0 / K, 1e-20, 1e20)] + [(s, 1.0, True) for s in (1.0 / K, 1e20)]
    rows = plane_rows(H)
    photon = _hostile_rows(np.zeros((rows, W, 4), f32), H)
    return SimpleNamespace(family=family, W=W, H=H, variant=variant, rows=rows, schedule=tuple(schedule), K=K, B=len(schedule),
                           states=[_plane(s, H, W) for s in states], photon=photon, light=_plane(light, H, W), mask=mask, calls=calls, marks=marks)


def sums_of(case):
    """the fp32 sums c = vpl + photon at every fold boundary, image rows only, keyed by the iteration count (numpy_variance's cs)"""
    cum = np.concatenate([[0], np.cumsum(case.schedule)])
    return {int(n): (s[:case.H, :, :3] + case.photon[:case.H, :, :3]).astype(f32) for n, s in zip(cum, case.states)}


def host_composite(case, scale, light_scale=1.0, mask_emitter=False, gamma=False):
    """resolve_kernel's expression in numpy (fp32, (H, W, 3)): what evplp_resolve(scale, scale, light_scale, mask_emitter) returns, up to the
    contraction the resolve's unit is compiled with -- the GPU tests take the downloaded composite instead"""
    with np.errstate(all="ignore"):
        vs, ls = f32(scale), f32(light_scale)
        l = case.light[:case.H, :, :3]
        step = np.where(f32(0) < l[..., :1] * ls, f32(0), f32(1)) if mask_emitter else f32(1)
        rgb = (step * (case.states[-1][:case.H, :, :3] * vs + case.photon[:case.H, :, :3] * vs) + l * ls).astype(f32)
        return np.power(rgb, f32(1.0 / 2.2)).astype(f32) if gamma else rgb


# ---- the shared restatement, with the rule
def restate(case, scale, light_scale, mask_emitter, composite, light=None):
    """var (H, W, 3) fp64 (evplp_noise_variance's image before the rounding to fp32), v, the three figures of evplp_noise_estimate and the
    tile figures of evplp_adaptive_tile_noise for an ACTIVE context (no tile records)"""
    light = case.light[:case.H] if light is None else light
    with np.errstate(all="ignore"):
        var, v = numpy_variance(sums_of(case), case.schedule, scale, with_v=True)
        figs = numpy_figures(var, composite, light, light_scale, mask_emitter, case.mask, v=v)
        num, rel = rel_of(var, composite, light, light_scale, mask_emitter, v=v)
        tiles = tile_means(rel, case.W, case.H)
    return SimpleNamespace(var=var, v=v, figs=figs, num=num, rel=rel, tiles=tiles)


MUTATIONS = ("no_clamp", "S_double", "kj_for_K", "B_for_B1", "mask_not_flipped", "emitter_without_scale", "broken_counted", "broken_num_zero")


def mutant(case, scale, light_scale, mask_emitter, composite, mut=None):
    """restate() written out once more with one thing wrong (mut of MUTATIONS; None: nothing wrong, and then it must equal restate() to the
    bit -- tests/test_stats_hostile_host.py checks that, so a mutant differs from the restatement by its mutation alone)"""
    cs, light = sums_of(case), case.light[:case.H]
    with np.errstate(all="ignore"):
        prev = cs[0]; q = np.zeros(prev.shape, f64); it = 0
        for k in case.schedule:
            it += k
            d = (cs[it] - prev).astype(f32).astype(f64)
            q = q + d * d / f64(k)
            prev = cs[it]
        K, B = float(case.K), float(case.B)
        s = (prev.astype(f64) - cs[0].astype(f64)) if mut == "S_double" else (prev - cs[0]).astype(f32).astype(f64)
        v = (q - s * s / (float(case.schedule[-1]) if mut == "kj_for_K" else K)) / (B if mut == "B_for_B1" else B - 1.0)
        s2K = f64(f32(scale)) ** 2 * K
        var = s2K * (v if mut == "no_clamp" else np.where(v > 0.0, v, 0.0))
        num = (var[..., 0] + var[..., 1]) + var[..., 2]
        emitter = np.zeros(num.shape, bool)
        if mask_emitter:
            emitter = f32(0.0) < (light[..., 0] if mut == "emitter_without_scale" else light[..., 0] * f32(light_scale))
            num = np.where(emitter, 0.0, num)
        cp = composite.astype(f64)
        den = ((cp[..., 0] * cp[..., 0] + cp[..., 1] * cp[..., 1]) + cp[..., 2] * cp[..., 2]) + 0.001
        broken = ~np.isfinite(den) | (~np.isfinite(v).all(-1) & ~emitter)
        sound_num = num
        num = np.where(broken, np.nan, num)
        rel = num / den
        if mut == "broken_num_zero":            # the old way: a NaN v has read 0 through the clamp, and den decides alone
            num = sound_num; rel = num / den
        keep = np.ones(num.shape, bool) if case.mask is None else (case.mask if mut == "mask_not_flipped" else case.mask[::-1]).any(-1)
        kept = int(keep.sum())
        figs = (num.sum() / num.size, rel.sum() / num.size, (rel[keep].sum() / kept if kept else 0.0))
        if mut == "broken_counted":
            tiles = _tiles_old(np.where(broken, 0.0, rel), case.W, case.H)
        else:
            tiles = tile_means(rel, case.W, case.H)
    return SimpleNamespace(var=var, v=v, figs=figs, num=num, rel=rel, tiles=tiles)


def _tiles_old(rel, W, H):
    """a tile's sum of rel over every in-image pixel, broken or not, over their count"""
    TX, TY = tiles_of(W, H)
    out = np.zeros((TY, TX), f64)
    for ty in range(TY):
        for tx in range(TX):
            t = rel[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
            out[ty, tx] = t.sum() / t.size
    return out


def old_tiles(case, scale, light_scale, mask_emitter, composite):
    """the tile figures as the kernels formed them before the rule: a NaN v read 0 through the clamp, a non-finite den went into the quotient,
    and every in-image pixel was counted -- the NaN that evplp_plan_budgets refuses"""
    light = case.light[:case.H]
    with np.errstate(all="ignore"):
        var = numpy_variance(sums_of(case), case.schedule, scale)
        num = (var[..., 0] + var[..., 1]) + var[..., 2]
        if mask_emitter:
            num = np.where(f32(0.0) < light[..., 0] * f32(light_scale), 0.0, num)
        cp = composite.astype(f64)
        den = ((cp[..., 0] * cp[..., 0] + cp[..., 1] * cp[..., 1]) + cp[..., 2] * cp[..., 2]) + 0.001
        return _tiles_old(num / den, case.W, case.H), num / den


# ---- the independent float64 statement
def statement_broken(states, hidden):
    """(H, W): by its sums alone a pixel's v is not finite -- a non-finite sum at a fold boundary, or a difference beyond fp32 (the library's
    D and S are fp32).  hidden: pixels that read no moments.  states: planes or (H, W, 3) images."""
    H, W = hidden.shape
    with np.errstate(all="ignore"):
        c = np.stack([np.asarray(s)[:H, :, :3] for s in states]).astype(f64)
        bad = ~np.isfinite(c).all(0)
        bad |= (np.abs(np.diff(c, axis=0)) > FLT_MAX).any(0) | (np.abs(c[-1] - c[0]) > FLT_MAX)
    return bad.any(-1) & ~hidden


def statement64(case, scale, light_scale, mask_emitter, composite, light=None, shards=None, s2K=None):
    """float64, from the batch means: var and its bar per channel, the broken set, the three figures with their bars, the tile means with
    theirs.  shards: [(the fp32 sums at a tracker's fold boundaries, in order, their k_j)], default the case's one; several (the iterations
    partition's pooled moments) pool their batches, and S is the sum of the shards' own fp32 S, so the bar takes sum |S_r| for |S|.
    s2K: the factor on s2 when it is not scale^2 K -- a retired or budget-mode tile's ((scale N) / n_t)^2 K_t, with the tile's own batches as
    the shard"""
    H, W = case.H, case.W
    light = case.light[:H] if light is None else light
    shards = [(list(sums_of(case).values()), case.schedule)] if shards is None else shards
    k = np.concatenate([np.asarray(sch, f64) for _, sch in shards])
    K, B = k.sum(), float(len(k))
    with np.errstate(all="ignore"):
        cs = [np.stack(s).astype(f64) for s, _ in shards]    # [B_r + 1, H, W, 3] each
        D = np.concatenate([np.diff(c, axis=0) for c in cs])
        kk = k[:, None, None, None]
        mj = D / kk
        m = D.sum(0) / K
        s2 = (kk * (mj - m) ** 2).sum(0) / (B - 1.0)
        s2K = f64(f32(scale)) ** 2 * K if s2K is None else s2K
        var = s2K * s2
        Q, S = (D * D / kk).sum(0), sum(np.abs(c[-1] - c[0]) for c in cs)
        bar = 2.0 * 2.0 ** -23 * (Q + S * S / K) / (B - 1.0) * s2K
        emitter = (f32(0.0) < light[..., 0].astype(f32) * f32(light_scale)) if mask_emitter else np.zeros((H, W), bool)
        cp = composite.astype(f64)
        den = (cp * cp).sum(-1) + 0.001
        broken = ~np.isfinite(composite).all(-1)
        for s, _ in shards:
            broken = broken | statement_broken(s, emitter)
        num = np.where(emitter, 0.0, var.sum(-1)); nbar = np.where(emitter, 0.0, bar.sum(-1))
        num = np.where(broken, np.nan, num); nbar = np.where(broken, 0.0, nbar)
        rel, rbar = num / den, np.where(broken, 0.0, nbar / den)
        keep = np.ones((H, W), bool) if case.mask is None else (case.mask[::-1] != 0).any(-1)
        n, kept = float(H * W), int(keep.sum())
        figs = (num.sum() / n, rel.sum() / n, rel[keep].sum() / kept if kept else 0.0)
        fbars = [nbar.sum() / n, rbar.sum() / n, rbar[keep].sum() / kept if kept else 0.0]
        fbars = tuple(b + 1e-12 * abs(f) if np.isfinite(f) else 0.0 for b, f in zip(fbars, figs))
        TX, TY = tiles_of(W, H)
        tiles, tbars = np.zeros((TY, TX), f64), np.zeros((TY, TX), f64)
        for ty in range(TY):
            for tx in range(TX):
                sl = (slice(8 * ty, 8 * ty + 8), slice(8 * tx, 8 * tx + 8))
                ok = ~broken[sl]
                if ok.any():
                    tiles[ty, tx] = rel[sl][ok].sum() / ok.sum()
                    tbars[ty, tx] = rbar[sl][ok].sum() / ok.sum() + 1e-12 * tiles[ty, tx]
    return SimpleNamespace(var=var, bar=bar, broken=broken, emitter=emitter, figs=figs, fig_bars=fbars, tiles=tiles, tile_bars=tbars, den=den)


def broken_per_tile(broken):
    H, W = broken.shape
    TX, TY = tiles_of(W, H)
    return np.array([[int(broken[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].sum()) for tx in range(TX)] for ty in range(TY)])


def in_image_per_tile(W, H):
    return broken_per_tile(np.ones((H, W), bool))


# ---- comparisons
def to32(var):
    """the fp64 variance as evplp_noise_variance stores it: rounded to fp32, Inf beyond it"""
    with np.errstate(over="ignore"):
        return np.asarray(var).astype(f32)


def same_nan(a, b):
    """the variance image's bytes, any NaN standing for any other (a NaN's sign and payload are not the library's to promise)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.where(np.isnan(a), f32(0), a).tobytes() == np.where(np.isnan(b), f32(0), b).tobytes()


def figure_ratio(got, want, bar):
    """|got - want| / bar for finite figures (0 / 0 = 0); a non-finite `want` must be met exactly (NaN by NaN): 0 if so, inf if not"""
    if not np.isfinite(want):
        return 0.0 if (np.isnan(got) if np.isnan(want) else got == want) else np.inf
    if not np.isfinite(got):
        return np.inf
    e = abs(got - want)
    return 0.0 if e == 0.0 else (e / bar if bar > 0 else np.inf)


def worst_ratio(got, want, bars):
    return max(figure_ratio(g, w, b) for g, w, b in zip(np.ravel(got), np.ravel(want), np.ravel(bars)))


def variance_ratio(var32, ref):
    """the worst |var - var_ref| / bar over the sound pixels' channels (fp32 image against statement64; its rounding to fp32 is inside the
    bar's factor 2 only where var is not tiny against the bar, so half an fp32 ulp of var is added)"""
    with np.errstate(all="ignore"):
        ok = ~ref.broken[..., None] & np.isfinite(var32) & np.isfinite(ref.var) & (ref.var < FLT_MAX)
        e = np.abs(var32.astype(f64) - ref.var)
        bar = ref.bar + 2.0 ** -24 * np.abs(ref.var) + 1e-45
        r = np.where(ok, np.where(e == 0.0, 0.0, e / bar), 0.0)
    return float(r.max())


def pick_tau(means, bars, exclude=None):
    """tau in the middle of the widest gap between sorted tile means; (tau, the gap, the larger bar of the two neighbours)"""
    flat = means.ravel(); order = np.argsort(flat)
    m, b = flat[order], bars.ravel()[order]
    gaps = np.diff(m)
    j = int(np.argmax(gaps))
    return 0.5 * (m[j] + m[j + 1]), float(gaps[j]), float(max(b[j], b[j + 1]))


# ---- frame error: hostile references for evplp_frame_error
def error_references(W, H, seed=0):
    """(name, reference (H, W, 3) fp32 top-down, mask or None): zeros, 1e20, Inf and NaN pixels; where a mask is given it keeps the hostile
    pixels out, so the third figure stays finite while the first two do not"""
    rng = np.random.default_rng([W, H, seed, 7])
    base = rng.random((H, W, 3)).astype(f32) + f32(0.05)
    out = []
    z = base.copy(); z[0, 0] = 0.0; z[H - 1, W - 1] = 0.0; z[H // 2, :, 1] = 0.0
    out.append(("zeros", z, None))
    for name, value in (("1e20", f32(1e20)), ("inf", f32(np.inf)), ("nan", f32(np.nan)), ("-inf", f32(-np.inf))):
        r = base.copy(); r[H - 1, W - 2, 1] = value; r[0, W - 1, 2] = value
        mask = np.full((H, W, 3), 255, np.uint8); mask[H - 1, W - 2] = 0; mask[0, W - 1] = 0; mask[1, 0, 0] = 0; mask[1, 0, 2] = 0
        out.append((name, r, mask)); out.append((name + "-unmasked", r, None))
    return out


# ---- the device
def upload_case(evplp, c, case):
    """tracking started on states[0], one fold per later state; works on a Context and on a Group"""
    assert c.local_rows == case.rows if hasattr(c, "local_rows") else True
    c.upload(evplp.BUF_LIGHT, case.light)
    c.upload(evplp.BUF_PHOTON_ACCUM, case.photon)
    c.upload(evplp.BUF_VPL_ACCUM, case.states[0])
    c.noise_track(True, case.mask)
    for k, s in zip(case.schedule, case.states[1:]):
        c.upload(evplp.BUF_VPL_ACCUM, s)
        c.noise_fold(k)


def estimates(c, case):
    """per call of case.calls: the figures, the composite and the variance image the device gives (image rows)"""
    out = []
    for scale, ls, me in case.calls:
        out.append(SimpleNamespace(scale=scale, ls=ls, me=me, figs=c.noise_estimate(scale, ls, mask_emitter=me),
                                   composite=c.resolve(scale, scale, ls, mask_emitter=me)[:case.H], var=c.noise_variance(scale)[:case.H]))
    return out
