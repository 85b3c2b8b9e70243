"""Does retiring converged tiles pay (evplp_group_adaptive_*)?  One JSON line at the end of stdout.

Config #2 of BASELINE on the furnished stand-in (evplp_synth_scene, style "hard", 331 k triangles), one rank: 1024 x 1024, Instant
Radiosity (1024 VPL paths, 3 bounces, misMode one, no photon splat).  Every run folds the noise tracker after each iteration.
  * reference: a long plain run (--ref-iters) in the same process; its composite is the reference of evplp_group_frame_error.
  * curves: a plain run and adaptive runs at each --taus value (tileRelMse), --iters iterations each, retiring every --every iterations with
    the loop's 1 / i scale after --min-batches folds.  Every --every iterations: the wall time of the run so far (host clock around
    synchronised iterations; the measurements themselves are not counted), relMSE against the reference, tiles retired, and the gather pass's
    own time (pass statistics) of that iteration.
  * where noise sits relative to cost: per run, the fraction of tiles retired against the fraction of gather time saved at the end -- a
    saving smaller than the retired fraction means the cheap tiles converged first.
  * floor: the gather call with every tile retired (tileRelMse huge), its pass time and its host wall time, against a full gather's.

--technique pt: the same questions for the path tracer in path-trace mode (evplp_group_adaptive_enable_pt), 3 bounces, one sample per pixel
per call, on the same scene.  Curves and reference as above with the path-tracing pass in the gather's place; then, with a plain group and an
adaptive group alternating call by call in this process (--calls each; host clock around a synchronised call, and the pass's own time;
median and p10 - p90):
  * floor: a call with every tile retired against a plain call;
  * active: call time at about 100 / 50 / 25 / 10 / 5 % active tiles (tileRelMse taken from the quantiles of the tile means after four
    samples); its first row is a control with adaptivity off on both groups.
--plain-calls N: nothing but N plain path-tracing calls, timed the same way (for a side-by-side of two builds of the library, EVPLP_LIB).
--pair-calls N: nothing but N pairs evplp_primary + evplp_path_trace in path-trace mode with nothing retired (the same, for two checkouts).
--samples-per-call 4,16: the per-sample time of evplp_path_trace_batch against the active fraction, beside the pair's; prints it and ends.
--curve-batch S: the curves (not the reference) run S iterations per call through evplp_path_trace_batch; --no-tables: the curves only.
--budget (photonfam): gather budget mode (evplp_adaptive_enable(.., 2)) against the plain run and binary retirement, one group per run, the
  runs alternating iteration by iteration in this process; a fold every iteration; relMSE against the plain reference of --ref-iters.
  Runs: plain; tileRelMse at each --taus value (retiring every --every iterations after --min-batches folds); budgets with window
  --budget-window (16), minSamples 1, at each --budget-quantiles (1,0.9), planned every window iterations after --min-batches folds.  The
  plain run goes --iters iterations, the others until they pass its final relMSE or 2 x --iters.  Then --calls calls each, alternating: a
  budget-mode gather with every budget full against a plain gather (host wall time around a synchronised call, and the pass's own time).
--technique pt --budget: budget mode (evplp_adaptive_enable_pt(.., 2)) against the plain batched run and binary retirement, one group per run, the
  runs alternating call by call in this process: S = --curve-batch (16) samples per call, a fold per call, a plan (or a retirement) every
  --every (16) iterations after --min-batches (4) folds; relMSE against a plain run of --ref-iters samples of other seeds.  Runs: plain;
  tileRelMse --budget-tau (0.005); budgets with minSamples 1 at each --budget-quantiles (1,0.95,0.9).  The plain run goes --iters
  iterations, the others until they pass its final relMSE or 3 x --iters.  Then the cost of the mode itself, --calls each: a budget-mode
  call with every budget full against a plain batch; the budget-mode fold against the frozen fold of mode 1; one tile-noise + plan +
  set-budgets round.

usage: python tools/adaptive_convergence.py [--technique photonfam|pt] [--iters N] [--ref-iters N] [--taus 0.002,0.0005] [--every N]
                                            [--min-batches N] [--calls N] [--plain-calls N]"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402,F401  (first, so libevplp_hip.so binds to the HIP runtime torch loaded)
import numpy as np  # noqa: E402
import evplp_amd as ev  # noqa: E402
import scenes  # noqa: E402

W, H, NL, NV, P = 1024, 1024, 1024, 1024, 4


class Runner:
    def __init__(self, g, sd, total):
        self.g, self.sd, self.total = g, sd, total
        self.js = ev.jitter_sequence(0, 4096, W, H)

    def iteration(self, i):
        fp = ev.frame_params(camera_pos=self.sd.cam_origin, mis_mode="one", clamping_value=1.0 / self.total, num_light_paths=NL,
                             num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=i, jitter=tuple(float(x) for x in self.js[i]))
        self.g.primary(tuple(self.js[i])); self.g.trace_light_paths(i); self.g.gather(fp, 0)


class PtRunner:
    """one path-traced sample per pixel per iteration (the pt technique's loop: jitter i, seed i, 3 bounces)"""
    def __init__(self, g, sd):
        self.g, self.sd = g, sd
        self.js = ev.jitter_sequence(0, 4096, W, H)

    def iteration(self, i):
        self.g.primary(tuple(self.js[i % len(self.js)])); self.g.path_trace(self.sd.cam_origin, i, 3)

    def batch(self, i, S):
        """iterations i .. i + S - 1 as one evplp_path_trace_batch: the same jitters and seeds, the same bits"""
        js = np.array([self.js[(i + k) % len(self.js)] for k in range(S)], np.float32)
        self.g.path_trace_batch(self.sd.cam_origin, js, np.arange(i, i + S, dtype=np.uint32), 3)


PASS = ev.PASS_GATHER_VPL          # the pass whose work retirement saves (main() switches it for --technique pt)


def gather_ms(g):
    return g.context(0).pass_stats(PASS)["ms"]


def spread(v):
    q = statistics.quantiles(v, n=10)
    return {"median": statistics.median(v), "p10": q[0], "p90": q[-1]}


def timed_calls(groups, sd, first, calls):
    """`calls` path-tracing calls on each group in turn (alternating call by call): host wall time around a synchronised call, and the pass time"""
    out = [{"wall": [], "pass": []} for _ in groups]
    for i in range(first, first + calls):
        for g, o in zip(groups, out):
            g.synchronize()
            t0 = time.perf_counter()
            g.path_trace(sd.cam_origin, i, 3); g.synchronize()
            o["wall"].append((time.perf_counter() - t0) * 1e3); o["pass"].append(gather_ms(g))
    return [{"wall_ms": spread(o["wall"]), "pass_ms": spread(o["pass"])} for o in out]


def tile_means_of(g, n):
    """per-tile mean relative variance of the composite at 1 / n, as evplp_adaptive_retire forms it (numpy, not bit for bit: for quantiles)"""
    s = 1.0 / n
    var = g.noise_variance(s).astype(np.float64).sum(-1)
    c = g.resolve(s, s, 1.0).astype(np.float64)
    rel = var / ((c * c).sum(-1) + 0.001)
    return rel.reshape(H // 8, 8, W // 8, 8).mean(axis=(1, 3))


def pt_tables(g, plain, sd, tiles, calls):
    """the floor and the active-fraction table: g adaptive, `plain` a second group without adaptivity, alternating"""
    runs = {"adaptive": PtRunner(g, sd), "plain": PtRunner(plain, sd)}
    rows = []
    for want in (None, 1.0, 0.5, 0.25, 0.10, 0.05, 0.0):       # None: the control -- both groups plain (what two groups differ by on their own)
        for name, grp in (("adaptive", g), ("plain", plain)):
            grp.clear_accumulators(); grp.noise_track(True)
            if name == "adaptive" and want is not None:
                grp.adaptive_enable(True, path_trace=True)
            for i in range(4):
                runs[name].iteration(i); grp.noise_fold(1)
        tau = 1e300 if want == 0.0 else (-1.0 if want in (None, 1.0) else float(np.quantile(tile_means_of(g, 4), 1.0 - want)))
        retired = g.adaptive_retire(0.25, tau, 2) if tau >= 0.0 else 0
        g.primary(tuple(runs["adaptive"].js[4])); plain.primary(tuple(runs["plain"].js[4]))
        a, p = timed_calls([g, plain], sd, 4, calls)
        rows.append({"adaptivity": want is not None, "active_fraction": 1.0 - retired / tiles, "adaptive": a, "plain": p,
                     "pass_fraction_of_plain": a["pass_ms"]["median"] / p["pass_ms"]["median"]})
        g.clear_accumulators(); g.adaptive_enable(False, path_trace=True)
    return rows[:-1], rows[-1]


def batch_table(g, sd, tiles, calls, sizes):
    """--samples-per-call: host wall time PER SAMPLE of a synchronised iteration against the fraction of active tiles -- through the pair of
    calls (primary + path_trace) and through evplp_path_trace_batch with S samples, alternating call by call in one process"""
    run = PtRunner(g, sd)
    cam = sd.cam_origin
    rows = []
    for want in (1.0, 0.5, 0.25, 0.10, 0.05):
        g.clear_accumulators(); g.noise_track(True); g.adaptive_enable(True, path_trace=True)
        for i in range(4):
            run.iteration(i); g.noise_fold(1)
        retired = g.adaptive_retire(0.25, float(np.quantile(tile_means_of(g, 4), 1.0 - want)), 2) if want < 1.0 else 0
        out = {"pair": []}
        out.update({f"batch_{S}": [] for S in sizes})
        i = 4
        for _ in range(calls):
            g.synchronize(); t0 = time.perf_counter()
            run.iteration(i); g.synchronize()
            out["pair"].append((time.perf_counter() - t0) * 1e3); i += 1
            for S in sizes:
                js = np.array([run.js[(i + k) % len(run.js)] for k in range(S)], np.float32)
                seeds = np.arange(i, i + S, dtype=np.uint32)
                g.synchronize(); t0 = time.perf_counter()
                g.path_trace_batch(cam, js, seeds, 3); g.synchronize()
                out[f"batch_{S}"].append((time.perf_counter() - t0) * 1e3 / S); i += S
        rows.append({"active_fraction": 1.0 - retired / tiles, "ms_per_sample": {k: spread(v) for k, v in out.items()}})
        g.clear_accumulators(); g.adaptive_enable(False, path_trace=True)
    return rows


def pair_calls(g, run, calls):
    """--pair-calls: `calls` synchronised pairs evplp_primary + evplp_path_trace in path-trace adaptive mode with nothing retired (the
    100 % row of the batch table), host wall time and the two passes' own times: uses only calls that the parent build has too"""
    g.clear_accumulators(); g.noise_track(True); g.adaptive_enable(True, path_trace=True)
    for i in range(4):
        run.iteration(i); g.noise_fold(1)
    wall, pt, pr = [], [], []
    for i in range(4, 4 + calls):
        g.synchronize(); t0 = time.perf_counter()
        run.iteration(i); g.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        pt.append(g.context(0).pass_stats(ev.PASS_PATH_TRACE)["ms"]); pr.append(g.context(0).pass_stats(ev.PASS_PRIMARY)["ms"])
    checksum = float(g.resolve(1.0, 0.0, 0.0).astype(np.float64).sum())
    g.clear_accumulators(); g.adaptive_enable(False, path_trace=True)
    return {"wall_ms": spread(wall), "path_trace_pass_ms": spread(pt), "primary_pass_ms": spread(pr), "accumulator_sum": checksum}


def curve(g, run, iters, every, tau, min_batches, tiles, S=1):
    g.clear_accumulators(); g.noise_track(True)
    if tau is not None:
        g.adaptive_enable(True, path_trace=PASS == ev.PASS_PATH_TRACE)
    g.synchronize()
    wall = 0.0; pts = []; retired = 0; gms = []
    for i in range(S - 1, iters, S):                             # i: the last iteration of this step (S = 1: every iteration)
        t0 = time.perf_counter()
        if S == 1:
            run.iteration(i); g.noise_fold(1)
        else:
            run.batch(i - S + 1, S); g.noise_fold(S)
        if tau is not None and (i + 1) % every == 0:
            retired += g.adaptive_retire(1.0 / (i + 1), tau, min_batches)
        g.synchronize()
        wall += (time.perf_counter() - t0) * 1e3
        gms.append(gather_ms(g) / S)
        if (i + 1) % every == 0:
            s = 1.0 / (i + 1)
            e = g.frame_error(s, s, 1.0)
            pts.append({"iteration": i + 1, "wall_ms": wall, "rel_mse": e[1], "retired_tiles": retired,
                        "gather_ms": statistics.median(gms[-(every // S):])})
    return pts, retired


def budget_runs(groups, sd, iters, every, min_batches, S, tau, quantiles):
    """--budget: every run on its own group (reference already set), alternating one call at a time"""
    runs = [{"name": "plain", "g": groups[0], "mode": None}, {"name": f"tileRelMse_{tau:g}", "g": groups[1], "mode": "binary"}]
    runs += [{"name": f"budget_q{q:g}", "g": groups[2 + k], "mode": "budget", "q": q} for k, q in enumerate(quantiles)]
    for r in runs:
        g = r["g"]
        g.clear_accumulators(); g.adaptive_enable(False); g.noise_track(True)
        if r["mode"] == "binary":
            g.adaptive_enable(True, path_trace=True)
        if r["mode"] == "budget":
            g.adaptive_enable(True, budget=True)
        g.synchronize()
        r.update(run=PtRunner(g, sd), wall=0.0, n=0, folds=0, points=[], done=False, samples=0, next_samples=g.adaptive_tiles().size * S if r["mode"] == "budget" else None)
    target = None
    while not all(r["done"] for r in runs):
        for r in runs:
            if r["done"]:
                continue
            g = r["g"]
            t0 = time.perf_counter()
            r["run"].batch(r["n"], S); g.noise_fold(S)
            r["n"] += S; r["folds"] += 1
            if r["mode"] == "budget":
                r["samples"] += r["next_samples"]
            if r["n"] % every == 0 and r["folds"] >= min_batches:
                if r["mode"] == "binary":
                    g.adaptive_retire(1.0 / r["n"], tau, min_batches)
                if r["mode"] == "budget":
                    b = ev.plan_budgets(g.adaptive_tile_noise(1.0 / r["n"]), g.adaptive_tiles(), S, 1, 0.0, r["q"])
                    g.adaptive_set_budgets(b); r["next_samples"] = int(b.sum())
            g.synchronize()
            r["wall"] += (time.perf_counter() - t0) * 1e3
            if r["n"] % every == 0:
                s = 1.0 / r["n"]
                p = {"iteration": r["n"], "wall_ms": r["wall"], "rel_mse": g.frame_error(s, s, 1.0)[1]}
                if r["mode"] == "budget":
                    p["tile_samples"] = r["samples"]; p["next_call_samples"] = r["next_samples"]
                if r["mode"] == "binary":
                    p["active_tiles"] = int((g.adaptive_tiles() == r["n"]).sum())
                r["points"].append(p)
            if r["name"] == "plain":
                r["done"] = r["n"] >= iters
                if r["done"]:
                    target = r["points"][-1]["rel_mse"]
            else:
                r["done"] = r["n"] >= 3 * iters or (target is not None and r["n"] >= iters and r["points"] and r["points"][-1]["rel_mse"] <= target)
    out = {}
    for r in runs:
        hit = None
        for p0, p1 in zip([{"wall_ms": 0.0, "rel_mse": math.inf}] + r["points"], r["points"]):
            if p1["rel_mse"] <= target:
                t = 1.0 if not math.isfinite(p0["rel_mse"]) else (p0["rel_mse"] - target) / max(p0["rel_mse"] - p1["rel_mse"], 1e-300)
                hit = p0["wall_ms"] + t * (p1["wall_ms"] - p0["wall_ms"]); break
        out[r["name"]] = {"points": r["points"], "ms_to_plain_final_rel_mse": hit}
    return out, target


def gather_budget_runs(groups, sd, total, iters, every, min_batches, taus, window, quantiles):
    """--budget (photonfam): every run on its own group (reference already set), alternating one iteration at a time"""
    runs = [{"name": "plain", "mode": None}] + [{"name": f"tileRelMse_{t:g}", "mode": "binary", "tau": t} for t in taus]
    runs += [{"name": f"budget_q{q:g}", "mode": "budget", "q": q} for q in quantiles]
    for r, g in zip(runs, groups):
        g.clear_accumulators(); g.adaptive_enable(False); g.noise_track(True)
        if r["mode"] == "binary":
            g.adaptive_enable(True)
        if r["mode"] == "budget":
            g.adaptive_enable(True, gather_budget=True); g.adaptive_budget_window(window)
        g.synchronize()
        r.update(g=g, run=Runner(g, sd, total), wall=0.0, n=0, points=[], done=False, gms=[], calls=0)
    ntiles = ((W + 7) // 8) * ((H + 7) // 8)
    target = None
    while not all(r["done"] for r in runs):
        for r in runs:
            if r["done"]:
                continue
            g = r["g"]
            t0 = time.perf_counter()
            r["run"].iteration(r["n"]); g.noise_fold(1)
            r["n"] += 1
            if r["mode"] == "binary" and r["n"] % every == 0:
                g.adaptive_retire(1.0 / r["n"], r["tau"], min_batches)
            if r["mode"] == "budget" and r["n"] % window == 0 and r["n"] >= min_batches:
                b = ev.plan_budgets(g.adaptive_tile_noise(1.0 / r["n"]), g.adaptive_tiles(), window, 1, 0.0, r["q"])
                g.adaptive_set_budgets(b); r["next"] = int(b.sum())
            g.synchronize()
            r["wall"] += (time.perf_counter() - t0) * 1e3
            r["gms"].append(gather_ms(g))
            if r["n"] % every == 0:
                s = 1.0 / r["n"]
                p = {"iteration": r["n"], "wall_ms": r["wall"], "rel_mse": g.frame_error(s, s, 1.0)[1], "gather_ms": statistics.median(r["gms"][-every:])}
                if r["mode"] == "budget":
                    p["tile_calls"] = int(g.adaptive_tiles().sum()); p["window_tile_calls"] = r.get("next", ntiles * window)
                if r["mode"] == "binary":
                    p["active_tiles"] = int((g.adaptive_tiles() == r["n"]).sum())
                r["points"].append(p)
            if r["name"] == "plain":
                r["done"] = r["n"] >= iters
                if r["done"]:
                    target = r["points"][-1]["rel_mse"]
            else:
                r["done"] = r["n"] >= 2 * iters or (target is not None and r["n"] >= iters and r["points"] and r["points"][-1]["rel_mse"] <= target)
    out = {}
    for r in runs:
        hit = None
        for p0, p1 in zip([{"wall_ms": 0.0, "rel_mse": math.inf}] + r["points"], r["points"]):
            if p1["rel_mse"] <= target:
                t = 1.0 if not math.isfinite(p0["rel_mse"]) else (p0["rel_mse"] - target) / max(p0["rel_mse"] - p1["rel_mse"], 1e-300)
                hit = p0["wall_ms"] + t * (p1["wall_ms"] - p0["wall_ms"]); break
        out[r["name"]] = {"points": r["points"], "ms_to_plain_final_rel_mse": hit, "iterations": r["n"], "wall_ms": r["wall"],
                          "best_rel_mse": min(p["rel_mse"] for p in r["points"])}
    return out, target


def gather_budget_costs(g, plain, sd, total, calls):
    """--budget (photonfam): a budget-mode gather with every budget full against a plain gather, alternating call by call"""
    runs = (Runner(g, sd, total), Runner(plain, sd, total))
    g.clear_accumulators(); g.adaptive_enable(False); g.noise_track(True); g.adaptive_enable(True, gather_budget=True)
    plain.clear_accumulators(); plain.adaptive_enable(False); plain.noise_track(True)
    out = {"budget_full_call": {"wall": [], "pass": []}, "plain_call": {"wall": [], "pass": []}}
    for k in range(calls + 2):
        for name, grp, run in (("budget_full_call", g, runs[0]), ("plain_call", plain, runs[1])):
            grp.synchronize(); t0 = time.perf_counter()
            run.iteration(k); grp.synchronize()
            t1 = time.perf_counter()
            grp.noise_fold(1)
            if k >= 2:
                out[name]["wall"].append((t1 - t0) * 1e3); out[name]["pass"].append(gather_ms(grp))
    same = g.resolve(1.0, 0.0, 0.0).tobytes() == plain.resolve(1.0, 0.0, 0.0).tobytes()
    g.clear_accumulators(); g.adaptive_enable(False); plain.clear_accumulators()
    res = {k: {"wall_ms": spread(v["wall"]), "gather_pass_ms": spread(v["pass"])} for k, v in out.items()}
    res["accumulators_identical"] = same
    return res


def budget_costs(g, plain, sd, S, calls):
    """--budget: what the mode itself costs, alternating call by call: g in budget mode with every budget full, `plain` with adaptivity off"""
    runs = (PtRunner(g, sd), PtRunner(plain, sd))
    g.clear_accumulators(); g.adaptive_enable(False); g.noise_track(True); g.adaptive_enable(True, budget=True)
    plain.clear_accumulators(); plain.adaptive_enable(False); plain.noise_track(True)
    wall = {"budget_full_call": [], "plain_batch_call": [], "budget_fold": [], "plain_fold": [], "tile_noise_plan_set_round": []}
    n = 0
    for k in range(calls + 2):
        for name, grp, run in (("budget_full_call", g, runs[0]), ("plain_batch_call", plain, runs[1])):
            grp.synchronize(); t0 = time.perf_counter()
            run.batch(n, S); grp.synchronize()
            t1 = time.perf_counter()
            grp.noise_fold(S); grp.synchronize()
            t2 = time.perf_counter()
            if k >= 2:
                wall[name].append((t1 - t0) * 1e3); wall["budget_fold" if grp is g else "plain_fold"].append((t2 - t1) * 1e3)
        n += S
        if k >= 2:
            t0 = time.perf_counter()
            b = ev.plan_budgets(g.adaptive_tile_noise(1.0 / n), g.adaptive_tiles(), S, 1, 0.0, 1.0)
            g.adaptive_set_budgets(np.full_like(b, S)); g.synchronize()          # (planned, then set full again: the next call stays a full one)
            wall["tile_noise_plan_set_round"].append((time.perf_counter() - t0) * 1e3)
    same = g.resolve(1.0, 0.0, 0.0).tobytes() == plain.resolve(1.0, 0.0, 0.0).tobytes()
    # the frozen fold of mode 1 (noise_fold_frozen_kernel), nothing retired
    plain.clear_accumulators(); plain.noise_track(True); plain.adaptive_enable(True, path_trace=True)
    frozen = []
    for k in range(calls + 2):
        runs[1].batch(k * S, S); plain.synchronize()
        t0 = time.perf_counter()
        plain.noise_fold(S); plain.synchronize()
        if k >= 2:
            frozen.append((time.perf_counter() - t0) * 1e3)
    plain.clear_accumulators(); plain.adaptive_enable(False, path_trace=True)
    g.clear_accumulators(); g.adaptive_enable(False, path_trace=True)
    out = {k: spread(v) for k, v in wall.items()}
    out["frozen_fold_mode_1"] = spread(frozen)
    out["accumulators_identical"] = same
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=128)
    ap.add_argument("--ref-iters", type=int, default=512)
    ap.add_argument("--taus", default="0.002,0.0005,0.0001")
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--min-batches", type=int, default=4)
    ap.add_argument("--technique", choices=("photonfam", "pt"), default="photonfam")
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--plain-calls", type=int, default=0)
    ap.add_argument("--samples-per-call", default="", help="pt: comma-separated batch sizes; prints the per-sample time table against the active fraction and ends")
    ap.add_argument("--curve-batch", type=int, default=1, help="pt: the curves run S iterations per call through evplp_path_trace_batch (S divides --every and --iters); "
                    "--min-batches then counts folds of S")
    ap.add_argument("--pair-calls", type=int, default=0, help="pt: nothing but N pairs primary + path_trace in path-trace mode, nothing retired (for two builds side by side)")
    ap.add_argument("--no-tables", action="store_true", help="pt: the curves only")
    ap.add_argument("--budget", action="store_true", help="budget mode against the plain run and binary retirement: the gathers', or with --technique pt the path tracer's (see the module text)")
    ap.add_argument("--budget-tau", type=float, default=0.005)
    ap.add_argument("--budget-quantiles", default="", help="default: 1,0.9 for the gathers, 1,0.95,0.9 for pt")
    ap.add_argument("--budget-window", type=int, default=16, help="--budget (photonfam): the window S")
    ap.add_argument("--no-curves", action="store_true", help="--budget: the cost table only")
    a = ap.parse_args()
    if not a.budget_quantiles:
        a.budget_quantiles = "1,0.95,0.9" if a.technique == "pt" else "1,0.9"
    if a.budget and a.technique == "pt":
        if a.curve_batch == 1:
            a.curve_batch, a.every = 16, 16
    assert a.curve_batch >= 1 and a.every % a.curve_batch == 0 and a.iters % a.curve_batch == 0, "--curve-batch must divide --every and --iters"
    pt = a.technique == "pt" or a.plain_calls > 0 or a.pair_calls > 0 or bool(a.samples_per_call)
    if pt:
        global PASS
        PASS = ev.PASS_PATH_TRACE
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    res = {"shape": {"W": W, "H": H, "numLightPaths": NL, "numVplLightPaths": NV, "scene": "hard, 331000 triangles"}, "tiles": tiles}
    with tempfile.TemporaryDirectory() as d:
        jp = ev.synth_scene(d, "conference_synth", 331000, 1234, W, H, style="hard")
        sd, _ = scenes.load_obj_scene(jp)
        with ev.Group(W, H, NL, NV, P, 1, devices=[0], overlap_light_tracing=True) as g:
            g.load_scene_json(jp)
            bsr, total, _ = g.context(0).scene_metrics()
            run = PtRunner(g, sd) if pt else Runner(g, sd, total)
            if a.samples_per_call:
                sizes = [int(x) for x in a.samples_per_call.split(",") if x]
                print(json.dumps({"library": ev.LIB_PATH, "shape": res["shape"], "tiles": tiles, "calls": a.calls, "batch_table": batch_table(g, sd, tiles, a.calls, sizes)}))
                return
            if a.pair_calls > 0:
                print(json.dumps({"library": ev.LIB_PATH, "pair_of_calls": pair_calls(g, run, a.pair_calls)}))
                return
            if a.budget and not pt:
                qs = [float(x) for x in a.budget_quantiles.split(",") if x]
                taus = [float(x) for x in a.taus.split(",") if x]
                res = {"library": ev.LIB_PATH, "shape": res["shape"], "tiles": tiles, "window": a.budget_window, "every": a.every, "min_batches": a.min_batches}
                others = []
                try:
                    for _ in range(1 if a.no_curves else len(taus) + len(qs)):
                        o = ev.Group(W, H, NL, NV, P, 1, devices=[0], overlap_light_tracing=True); o.load_scene_json(jp); others.append(o)
                    if not a.no_curves:
                        g.clear_accumulators()
                        for i in range(a.ref_iters):
                            run.iteration(i)
                        s = 1.0 / a.ref_iters
                        ref = np.ascontiguousarray(g.resolve(s, s, 1.0)[::-1]).astype(np.float32)
                        for grp in [g] + others:
                            grp.set_error_reference(ref)
                        res["reference_iterations"] = a.ref_iters
                        # (a plain run of iterations 0 .. ref_iters - 1, as the issue and DESIGN's earlier gather rows have it: every curve's
                        # samples are among the reference's, unlike the pt branch below, whose reference has seeds of its own)
                        res["reference_shares_samples_with_curves"] = True
                        res["runs"], res["plain_final_rel_mse"] = gather_budget_runs([g] + others, sd, total, a.iters, a.every, a.min_batches, taus, a.budget_window, qs)
                    res["costs"] = gather_budget_costs(g, others[0], sd, total, a.calls)
                finally:
                    for o in others:
                        o.close()
                print(json.dumps(res))
                return
            if a.budget:
                qs = [float(x) for x in a.budget_quantiles.split(",") if x]
                res = {"library": ev.LIB_PATH, "shape": res["shape"], "tiles": tiles, "samples_per_call": a.curve_batch, "every": a.every, "min_batches": a.min_batches}
                others = []
                try:
                    for _ in range(1 if a.no_curves else 1 + len(qs)):
                        o = ev.Group(W, H, NL, NV, P, 1, devices=[0]); o.load_scene_json(jp); others.append(o)
                    if not a.no_curves:
                        g.clear_accumulators()
                        for i in range(0, a.ref_iters, 16):
                            run.batch(i + (1 << 20), 16)                 # (samples of its own: no curve shares any with the reference)
                        s = 1.0 / a.ref_iters
                        ref = np.ascontiguousarray(g.resolve(s, s, 1.0)[::-1]).astype(np.float32)
                        for grp in [g] + others:
                            grp.set_error_reference(ref)
                        res["reference_iterations"] = a.ref_iters
                        res["runs"], res["plain_final_rel_mse"] = budget_runs([g] + others, sd, a.iters, a.every, a.min_batches, a.curve_batch, a.budget_tau, qs)
                    res["costs"] = budget_costs(g, others[0], sd, a.curve_batch, a.calls)
                finally:
                    for o in others:
                        o.close()
                print(json.dumps(res))
                return
            if a.plain_calls > 0:
                g.clear_accumulators()
                for i in range(4):
                    run.iteration(i)
                print(json.dumps({"library": ev.LIB_PATH, "plain_path_trace_call": timed_calls([g], sd, 4, a.plain_calls)[0]}))
                return
            # the reference: a long plain run
            g.clear_accumulators()
            for i in range(a.ref_iters):
                run.iteration(i + (1 << 20) if pt else i)        # (pt: samples of its own, so that no curve shares any with the reference)
            s = 1.0 / a.ref_iters
            ref = np.ascontiguousarray(g.resolve(s, s, 1.0)[::-1]).astype(np.float32)
            g.set_error_reference(ref)
            res["reference_iterations"] = a.ref_iters
            runs = {}
            for tau in [None] + [float(x) for x in a.taus.split(",") if x]:
                g.clear_accumulators()                           # (N = 0: adaptivity can be switched)
                g.adaptive_enable(False)
                pts, retired = curve(g, run, a.iters, a.every, tau, a.min_batches, tiles, a.curve_batch)
                name = "plain" if tau is None else f"tileRelMse_{tau:g}"
                runs[name] = {"points": pts, "retired_tiles": retired}
            g.clear_accumulators(); g.adaptive_enable(False)
            base = runs["plain"]["points"]
            for name, r in runs.items():
                last = r["points"][-1]
                r["retired_fraction"] = r["retired_tiles"] / tiles
                r["gather_time_saved_fraction"] = 1.0 - last["gather_ms"] / base[-1]["gather_ms"]
                # time to reach the plain run's final relMSE (linear interpolation between checkpoints; null when not reached)
                target = base[-1]["rel_mse"]
                hit = None
                for p0, p1 in zip([{"wall_ms": 0.0, "rel_mse": math.inf}] + r["points"], r["points"]):
                    if p1["rel_mse"] <= target:
                        t = 1.0 if not math.isfinite(p0["rel_mse"]) else (p0["rel_mse"] - target) / max(p0["rel_mse"] - p1["rel_mse"], 1e-300)
                        hit = p0["wall_ms"] + t * (p1["wall_ms"] - p0["wall_ms"]); break
                r["ms_to_plain_final_rel_mse"] = hit
            res["runs"] = runs
            res["curve_samples_per_call"] = a.curve_batch
            if pt and a.no_tables:
                print(json.dumps(res))
                return
            if pt:
                with ev.Group(W, H, NL, NV, P, 1, devices=[0]) as plain:
                    plain.load_scene_json(jp)
                    res["active"], res["floor"] = pt_tables(g, plain, sd, tiles, a.calls)
                print(json.dumps(res))
                return
            # the floor: every tile retired
            g.clear_accumulators(); g.noise_track(True); g.adaptive_enable(True)
            for i in range(4):
                run.iteration(i); g.noise_fold(1)
            full_pass = gather_ms(g)
            assert g.adaptive_retire(0.25, 1e300, 2) == tiles
            walls, passes = [], []
            for i in range(4, 24):
                g.synchronize()
                t0 = time.perf_counter()
                fp = ev.frame_params(camera_pos=sd.cam_origin, mis_mode="one", clamping_value=1.0 / total, num_light_paths=NL,
                                     num_vpl_light_paths=NV, photons_per_path=P, do_accumulate=1, rng_seed=i)
                g.gather(fp, 0); g.synchronize()
                walls.append((time.perf_counter() - t0) * 1e3); passes.append(gather_ms(g))
            res["floor"] = {"all_retired_gather_pass_ms": statistics.median(passes), "all_retired_gather_wall_ms": statistics.median(walls),
                            "full_gather_pass_ms": full_pass, "floor_fraction": statistics.median(passes) / full_pass}
            g.clear_accumulators(); g.adaptive_enable(False)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
