"""Gather budget mode without a GPU: the new entry points (exported, bound, declared, refusing null handles; the ABI version unchanged), what
include/evplp.h says about evplp_adaptive_enable(ctx, 2) and the window, and the "budget" object of photonfam's "adaptive" block -- validated
before any group exists, every parse error naming its key."""
import ctypes as C
import json
import os
import re

import pytest

from test_adaptive_host import GOOD, NOISE, _render, _technique_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_adaptive_budget_window", "evplp_group_adaptive_budget_window")


def test_new_entry_points_are_exported_bound_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    for p in ("", "group_"):
        assert getattr(L, f"evplp_{p}adaptive_budget_window")(None, 16) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}adaptive_enable")(None, 2) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for cls in (evplp.Context, evplp.Group):
        assert callable(getattr(cls, "adaptive_budget_window"))
        assert "gather_budget" in cls.adaptive_enable.__code__.co_varnames


def test_the_header_documents_the_mode_and_the_window():
    hdr = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "evplp.h")).read())
    for needle in ("2 = gather budget mode", "Gather budget mode: evplp_adaptive_enable(ctx, 2)", "evplp_adaptive_budget_window(ctx, S), S in 1 .. 64, 16 after entering",
                   "b_t < 0 || (m % S) < min(b_t, S)", "no evplp_splat_photons since the last clear", "with budgets never set the mode equals a plain run in every bit",
                   "evplp_group_adaptive_enable(g, 2)"):
        assert needle in hdr, needle


@pytest.fixture
def room(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, 96, 64)


def _with(budget, every=16, **tech):
    root = {"adaptive": dict(GOOD, budget=budget, everyIterations=every), "noise": dict(NOISE, everyIterations=every)}
    root.update(tech)
    return json.dumps(root)


def test_bad_budget_blocks_are_refused_before_any_gpu_work(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "photonfam")
    B = "adaptive.budget"
    cases = [
        (_with({}, every=8), ["adaptive.everyIterations", B + ".window"]),                # the default window is 16
        (_with({"window": 4}, every=6), ["adaptive.everyIterations", B + ".window"]),
        (_with({"window": 0}), [B + ".window"]),
        (_with({"window": 65}), [B + ".window"]),
        (_with({"window": "4"}), [B + ".window"]),
        (_with({"window": 4, "minSamples": 5}), [B + ".minSamples"]),
        (_with({"minSamples": 0}), [B + ".minSamples"]),
        (_with({"referenceQuantile": 0}), [B + ".referenceQuantile"]),
        (_with({"referenceQuantile": 1.5}), [B + ".referenceQuantile"]),
        (_with(3), [B]),
        # where the loop would splat photons: run.photonSplat with a photon radius
        (_with({}, radiusPercentage=0.05, run={"photonSplat": True}), [B, "photon"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    for f in ("noise.json", "iters.pfm"):
        assert not (tmp_path / f).exists(), f
    # lvcphotonfam takes no "adaptive" block, with or without a budget
    rc, msg = _render(evplp, _technique_file(room, tmp_path, "lvcphotonfam"), _with({}))
    assert rc == evplp.ERR_PARSE and "lvcphotonfam" in msg, (rc, msg)
    # pt's window is samplesPerCall
    rc, msg = _render(evplp, _technique_file(room, tmp_path, "pt"),
                      json.dumps({"adaptiveSampling": dict(GOOD, budget={"window": 4}), "noise": NOISE, "samplesPerCall": 2}))
    assert rc == evplp.ERR_PARSE and "adaptiveSampling.budget.window" in msg, (rc, msg)


def test_valid_budget_blocks_get_past_validation(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "photonfam")
    for budget, every, tech in (({}, 16, {}), ({"window": 4, "minSamples": 2, "referenceQuantile": 0.9}, 8, {}),
                                ({"window": 64}, 64, {}),
                                # photonSplat without a radius draws nothing, and a radius without the pass neither
                                ({"window": 4}, 4, {"radiusPercentage": 0, "run": {"photonSplat": True}}),
                                ({"window": 4}, 4, {"radiusPercentage": 0.05, "run": {"photonSplat": False}})):
        rc, msg = _render(evplp, jp, _with(budget, every=every, **tech))
        assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "budget" not in msg, (budget, rc, msg)
