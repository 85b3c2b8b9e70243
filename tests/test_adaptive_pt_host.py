"""Adaptive sampling for the path tracer without a GPU: the two additive entry points (exported, bound, declared, refusing null handles; the
ABI version unchanged), and the optional "adaptiveSampling" block of the pt technique -- validated completely before any group exists, so
that a bad block costs no GPU time and fails here with a parse error naming the key."""
import ctypes as C
import json
import os
import re

import pytest

from test_adaptive_host import GOOD, NOISE, _render, _technique_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_adaptive_enable_pt", "evplp_group_adaptive_enable_pt")
KEY = "adaptiveSampling"


def test_new_entry_points_are_exported_bound_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    for on in (0, 1):
        assert L.evplp_adaptive_enable_pt(None, on) == evplp.ERR_INVALID
        assert L.evplp_group_adaptive_enable_pt(None, on) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)


@pytest.fixture
def room(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, 96, 64)


def _block(noise=True, **kw):
    b = dict(GOOD)
    for k, v in kw.items():
        if v is None:
            b.pop(k)
        else:
            b[k] = v
    root = {KEY: b}
    if noise:
        root["noise"] = NOISE
    return json.dumps(root)


def test_bad_blocks_are_refused_before_any_gpu_work(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "pt")
    cases = [
        (_block(noise=False), [KEY, "noise"]),
        (_block(tileRelMse=None), [KEY + ".tileRelMse"]),
        (_block(tileRelMse=-1e-3), [KEY + ".tileRelMse"]),
        (_block(tileRelMse="0.1"), [KEY + ".tileRelMse"]),
        (_block(everyIterations=0), [KEY + ".everyIterations"]),
        (_block(everyIterations=5), [KEY + ".everyIterations", "multiple"]),
        (_block(minBatches=1), [KEY + ".minBatches"]),
        (_block(minBatches=0), [KEY + ".minBatches"]),
        (_block(iterationsFilename=3), [KEY + ".iterationsFilename"]),
        (json.dumps({KEY: 3, "noise": NOISE}), [KEY]),
        (json.dumps({KEY: GOOD, "noise": NOISE, "device": {"partition": "iterations"}}), [KEY, "iterations"]),
        (json.dumps({KEY: GOOD, "noise": NOISE, "frameMode": "cleareveryframe"}), [KEY, "cleareveryframe"]),
        (json.dumps({KEY: GOOD, "frameMode": "cleareveryframe"}), [KEY, "cleareveryframe"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    for f in ("noise.json", "iters.pfm", "pt.pfm"):                       # (pt.json is the technique file itself)
        assert not (tmp_path / f).exists(), f


def test_the_gather_key_inside_pt_points_to_the_new_one(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "pt")
    rc, msg = _render(evplp, jp, json.dumps({"adaptive": GOOD, "noise": NOISE}))
    assert rc == evplp.ERR_PARSE and "adaptive: not for pt" in msg and KEY in msg, (rc, msg)


def test_a_valid_block_gets_past_validation(evplp, room, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_adaptive_pt.py)")
    jp = _technique_file(room, tmp_path, "pt")
    rc_plain, msg_plain = _render(evplp, jp)
    rc, msg = _render(evplp, jp, _block())
    assert rc_plain < 0 and rc == rc_plain, (rc, msg, rc_plain, msg_plain)
    assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and KEY not in msg, msg
