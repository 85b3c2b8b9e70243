"""Budget mode of the path tracer without a GPU: evplp_plan_budgets against a numpy restatement (every budget equal) and its properties and
refusals; the new entry points (exported, bound, declared, refusing null handles; the ABI version unchanged); and the "budget" object of the
pt technique's "adaptiveSampling" block -- validated before any group exists, every parse error naming its key."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_adaptive_host import GOOD, NOISE, _render, _technique_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_adaptive_set_budgets", "evplp_adaptive_budgets", "evplp_adaptive_tile_noise", "evplp_group_adaptive_set_budgets",
       "evplp_group_adaptive_budgets", "evplp_group_adaptive_tile_noise", "evplp_plan_budgets")
KEY = "adaptiveSampling"


def test_new_entry_points_are_exported_bound_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    b = np.zeros(4, np.int32); d = np.zeros(4, np.float64)
    for p in ("", "group_"):
        assert getattr(L, f"evplp_{p}adaptive_set_budgets")(None, b.ctypes.data, 4) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}adaptive_budgets")(None, b.ctypes.data, 4) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}adaptive_tile_noise")(None, 1.0, 1.0, 0, d.ctypes.data, 4) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}adaptive_enable_pt")(None, 2) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for cls in (evplp.Context, evplp.Group):
        for m in ("adaptive_set_budgets", "adaptive_budgets", "adaptive_tile_noise"):
            assert callable(getattr(cls, m)), m
    assert callable(evplp.plan_budgets)


# ---- the planner

def plan_numpy(rel, n_t, samples, min_samples, tau, q):
    """include/evplp.h evplp_plan_budgets, restated: plain double arithmetic -- one division, one sqrt, one product, one ceil"""
    rel = np.asarray(rel, np.float64); n_t = np.asarray(n_t, np.int32)
    out = np.zeros(n_t.shape, np.int32)
    own = n_t > 0
    v = rel * n_t.astype(np.float64)
    srt = np.sort(v[own])
    m = srt.size
    v_ref = srt[min(m - 1, int(np.floor(q * m)))] if m else 0.0
    stop = own & (rel <= tau) if tau > 0 else np.zeros(own.shape, bool)
    go = own & ~stop
    if not v_ref > 0:
        out[go] = samples
        return out, None
    x = np.float64(samples) * np.sqrt(v / v_ref)
    s = np.clip(np.ceil(x), max(1, min_samples), samples).astype(np.int32)
    out[go] = s[go]
    # (the reference tile itself: v_t / v_ref is exactly 1 in any arithmetic and its x exactly `samples` -- nothing there for ceil to hide)
    return out, x[go & (v != v_ref)]


def draw(seed, n, samples, tau, q):
    """rel over four decades, some tiles with n_t = 0, some at or below tau, none whose samples * sqrt(v_t / v_ref) is within 1e-9 of an integer"""
    rng = np.random.default_rng(seed)
    for attempt in range(100):
        rel = 10.0 ** rng.uniform(-5.0, -1.0, n)
        n_t = rng.integers(4, 200, n).astype(np.int32)
        n_t[rng.random(n) < 0.1] = 0
        n_t[0], n_t[1], n_t[2] = 0, 16, 16                                # (every draw has a tile nobody owns ...)
        if tau > 0:
            at = rng.random(n) < 0.05
            at[1] = True
            rel[at] = tau                                                 # exactly at tau: stopped
            rel[2] = 0.5 * tau                                            # (... one at tau and one below it)
        _, x = plan_numpy(rel, n_t, samples, 1, tau, q)
        if x is not None and (np.abs(x - np.rint(x)) > 1e-9).all():
            return rel, n_t
    raise AssertionError("no draw clear of the integers")


@pytest.mark.parametrize("n", [91, 16384])
def test_the_planner_equals_its_numpy_restatement(evplp, n):
    cases = 0
    for seed in range(5):
        for samples in (1, 16, 64):
            for q in (1.0, 0.9):
                for mn in (1, 4):
                    if mn > samples:
                        continue
                    for tau in (0.0, 1e-3):
                        rel, n_t = draw(1000 * seed + n, n, samples, tau, q)
                        want, x = plan_numpy(rel, n_t, samples, mn, tau, q)
                        assert (np.abs(x - np.rint(x)) > 1e-9).all()      # ceil cannot hide a rounding difference
                        assert (n_t == 0).any() and (tau == 0 or (rel[n_t > 0] <= tau).any())
                        got = evplp.plan_budgets(rel, n_t, samples, mn, tau, q)
                        assert np.array_equal(got, want), (seed, samples, q, mn, tau, int((got != want).sum()))
                        cases += 1
    assert cases == 5 * (2 * 2 + 2 * 2 * 2 * 2)
    # v_ref = 0: every remaining tile gets `samples`; tiles nobody owns get 0
    rel = np.zeros(n); n_t = np.full(n, 8, np.int32); n_t[::7] = 0
    got = evplp.plan_budgets(rel, n_t, 16, 4, 0.0, 0.9)
    assert np.array_equal(got, np.where(n_t > 0, 16, 0)) and np.array_equal(got, plan_numpy(rel, n_t, 16, 4, 0.0, 0.9)[0])
    # ... and under q = 0.5 with the top twentieth alone noisy, v_ref is still 0
    rel[-(n // 20):] = 0.5
    assert np.array_equal(evplp.plan_budgets(rel, n_t, 16, 1, 0.0, 0.5), np.where(n_t > 0, 16, 0))


def test_planner_properties(evplp):
    rng = np.random.default_rng(5)
    n = 4096
    rel = 10.0 ** rng.uniform(-6.0, -1.0, n)
    n_t = np.full(n, 32, np.int32)
    n_t[rng.random(n) < 0.1] = 0
    for samples, mn, tau, q in ((16, 1, 0.0, 1.0), (16, 4, 1e-4, 0.9), (64, 0, 0.0, 0.5), (1, 1, 1e-3, 1.0), (5, 5, 0.0, 0.3)):
        b = evplp.plan_budgets(rel, n_t, samples, mn, tau, q)
        lo = max(1, mn)
        assert ((b == 0) | ((b >= lo) & (b <= samples))).all()            # {0} U [max(1, min), S]
        assert (b[n_t <= 0] == 0).all()
        own = n_t > 0
        stopped = own & (rel <= tau) if tau > 0 else np.zeros(n, bool)
        assert (b[stopped] == 0).all() and (b[own & ~stopped] >= lo).all()  # with tau = 0 no owned tile ever stops improving
        v = rel * n_t
        srt = np.sort(v[own])
        v_ref = srt[min(srt.size - 1, int(np.floor(q * srt.size)))]
        live = own & ~stopped
        assert (b[live & (v >= v_ref)] == samples).all()                  # at v_ref or above: the full rate
        order = np.argsort(v[live], kind="stable")
        assert (np.diff(b[live][order]) >= 0).all()                       # monotone in v_t


def test_planner_refusals(evplp):
    L = evplp.lib()
    rel = np.array([0.1, 0.2, 0.3]); n_t = np.array([4, 4, 4], np.int32); out = np.full(3, -7, np.int32)
    r, t, o = rel.ctypes.data, n_t.ctypes.data, out.ctypes.data

    def call(rel_p=r, nt_p=t, n=3, samples=16, mn=1, tau=0.0, q=1.0, out_p=o):
        return L.evplp_plan_budgets(rel_p, nt_p, n, samples, mn, C.c_double(tau), C.c_double(q), out_p)
    assert call() == evplp.OK and out.tolist() == [10, 14, 16]
    bad = [dict(samples=0), dict(samples=65), dict(samples=-1), dict(mn=-1), dict(mn=17), dict(q=0.0), dict(q=-0.5), dict(q=1.0000001), dict(q=float("nan")),
           dict(rel_p=None), dict(nt_p=None), dict(out_p=None), dict(n=0), dict(n=-3)]
    out[:] = -7
    for kw in bad:
        assert call(**kw) == evplp.ERR_INVALID, kw
    for v in (-1e-9, float("nan"), float("inf")):
        bad_rel = np.array([0.1, v, 0.3])
        assert call(rel_p=bad_rel.ctypes.data) == evplp.ERR_INVALID, v
    assert out.tolist() == [-7, -7, -7]                                   # a refused call writes nothing
    assert call(mn=0) == evplp.OK and call(mn=16) == evplp.OK and out.tolist() == [16, 16, 16]
    with pytest.raises(evplp.EvplpError):
        evplp.plan_budgets(rel, n_t, 0)
    with pytest.raises(ValueError):
        evplp.plan_budgets(rel, n_t[:2], 16)


def test_separate_processes_agree(evplp):
    code = ("import sys, numpy as np; sys.path.insert(0, %r); import evplp_amd as ev; r = np.random.default_rng(11);"
            "rel = 10.0 ** r.uniform(-5, -1, 16384); n = r.integers(0, 99, 16384).astype(np.int32);"
            "sys.stdout.write(ev.plan_budgets(rel, n, 16, 1, 1e-4, 0.95).tobytes().hex())") % ROOT
    outs = [subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300) for _ in range(2)]
    assert all(o.returncode == 0 for o in outs), outs[0].stderr[-2000:]
    assert outs[0].stdout == outs[1].stdout and len(outs[0].stdout) == 16384 * 8


# ---- the technique block

@pytest.fixture
def room(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, 96, 64)


def _with(budget, spc=2, **extra):
    root = {KEY: dict(GOOD, budget=budget), "noise": NOISE}
    if spc is not None:
        root["samplesPerCall"] = spc
    root.update(extra)
    return json.dumps(root)


def test_bad_budget_blocks_are_refused_before_any_gpu_work(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "pt")
    B = KEY + ".budget"
    cases = [
        (_with({}, spc=None), [B, "samplesPerCall"]),
        (_with({}, spc=1), [B, "samplesPerCall"]),
        (_with(3), [B]),
        (_with([1]), [B]),
        (_with("on"), [B]),
        (_with({"minSamples": 0}), [B + ".minSamples"]),
        (_with({"minSamples": 3}), [B + ".minSamples"]),                  # above samplesPerCall = 2
        (_with({"minSamples": -1}), [B + ".minSamples"]),
        (_with({"minSamples": "1"}), [B + ".minSamples"]),
        (_with({"referenceQuantile": 0}), [B + ".referenceQuantile"]),
        (_with({"referenceQuantile": 1.5}), [B + ".referenceQuantile"]),
        (_with({"referenceQuantile": -0.1}), [B + ".referenceQuantile"]),
        (_with({"referenceQuantile": "1"}), [B + ".referenceQuantile"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    for f in ("noise.json", "iters.pfm", "pt.pfm"):
        assert not (tmp_path / f).exists(), f


def test_the_gathers_block_takes_no_budget(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "photonfam")
    rc, msg = _render(evplp, jp, json.dumps({"adaptive": dict(GOOD, budget={}), "noise": NOISE}))
    assert rc == evplp.ERR_PARSE and "adaptive.budget" in msg, (rc, msg)


def test_valid_budget_blocks_get_past_validation(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "pt")
    for budget, tau in (({}, 0), ({"minSamples": 2, "referenceQuantile": 0.9}, 0.002), ({"minSamples": 1, "referenceQuantile": 1.0}, 0)):
        rc, msg = _render(evplp, jp, json.dumps({KEY: dict(GOOD, budget=budget, tileRelMse=tau), "noise": NOISE, "samplesPerCall": 2}))
        assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "budget" not in msg, (budget, rc, msg)
