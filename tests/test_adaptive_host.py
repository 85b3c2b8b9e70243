"""Adaptive gather without a GPU: the six additive entry points (exported, bound, declared, refusing null handles), the Python binding's
argument checks, and the optional "adaptive" block of the technique JSON -- validated completely before any group exists, so that a bad
block costs no GPU time and fails here with a parse error."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
NEW = ("evplp_adaptive_enable", "evplp_adaptive_retire", "evplp_adaptive_tiles",
       "evplp_group_adaptive_enable", "evplp_group_adaptive_retire", "evplp_group_adaptive_tiles")


def _render(evplp, path, overrides=None):
    err = C.create_string_buffer(1024)
    rc = evplp.lib().evplp_render_json(str(path).encode(), overrides.encode() if overrides else None, 0, err, 1024)
    return rc, err.value.decode()


def test_new_entry_points_are_exported_bound_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    tiles = np.zeros(96, np.int32)
    for p in ("", "group_"):
        assert getattr(L, f"evplp_{p}adaptive_enable")(None, 1) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}adaptive_retire")(None, 1.0, 1.0, 0, 0.01, 2) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}adaptive_tiles")(None, tiles.ctypes.data, tiles.size) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5


class _NoC:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} made before the arguments were checked")


@pytest.mark.parametrize("cls", ["Context", "Group"])
def test_python_checks_retire_arguments_before_any_c_call(evplp, cls):
    obj = object.__new__(getattr(evplp, cls))
    obj._lib = _NoC(); obj._h = None; obj.W, obj.H = W, H
    for tau, mb in [(-1e-3, 2), (float("nan"), 2), ("0.1", 2), (None, 2), (True, 2), (0.01, 1), (0.01, 0), (0.01, 2.5), (0.01, "3"), (0.01, True)]:
        with pytest.raises(ValueError):
            obj.adaptive_retire(0.5, tau, mb)


@pytest.fixture
def room(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, W, H)


NOISE = {"batchIterations": 2, "everyIterations": 4, "filename": "noise.json"}
GOOD = {"tileRelMse": 0.002, "everyIterations": 4, "minBatches": 3, "iterationsFilename": "iters.pfm"}


def _block(noise=True, **kw):
    b = dict(GOOD)
    for k, v in kw.items():
        if v is None:
            b.pop(k)
        else:
            b[k] = v
    root = {"adaptive": b}
    if noise:
        root["noise"] = NOISE
    return json.dumps(root)


def _technique_file(room, tmp_path, technique):
    root = json.load(open(room))
    if technique == "pt":
        root["pt"] = {"rngOffset": 0, "numMaxIteration": 2, "timeLimitMs": 1e9, "frameMode": "accumulate", "outputFilename": "pt.pfm",
                      "statFilename": "pt.json", "useJitter": True, "useStat": True, "numSamplePerPixel": 1, "numMaxBounces": 3}
        root.pop("photonfam")
    elif technique == "lvcphotonfam":
        root["lvcphotonfam"] = root.pop("photonfam")
    jp = tmp_path / f"{technique}.json"
    jp.write_text(json.dumps(root))
    return jp


def test_bad_adaptive_blocks_are_refused_before_any_gpu_work(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "photonfam")
    cases = [
        (_block(noise=False), ["adaptive", "noise"]),
        (_block(tileRelMse=None), ["adaptive.tileRelMse"]),
        (_block(tileRelMse=-1e-3), ["adaptive.tileRelMse"]),
        (_block(tileRelMse="0.1"), ["adaptive.tileRelMse"]),
        (_block(everyIterations=0), ["adaptive.everyIterations"]),
        (_block(everyIterations=5), ["adaptive.everyIterations", "multiple"]),
        (_block(minBatches=1), ["adaptive.minBatches"]),
        (_block(minBatches=0), ["adaptive.minBatches"]),
        (_block(iterationsFilename=3), ["adaptive.iterationsFilename"]),
        (json.dumps({"adaptive": 3, "noise": NOISE}), ["adaptive"]),
        (json.dumps({"adaptive": GOOD, "noise": NOISE, "device": {"partition": "iterations"}}), ["adaptive", "iterations"]),
        (json.dumps({"adaptive": GOOD, "noise": NOISE, "frameMode": "cleareveryframe"}), ["cleareveryframe"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    assert not (tmp_path / "noise.json").exists() and not (tmp_path / "iters.pfm").exists()


@pytest.mark.parametrize("technique", ["lvcphotonfam", "pt"])
def test_techniques_without_a_vpl_or_vsl_gather_refuse_the_block(evplp, room, tmp_path, technique):
    jp = _technique_file(room, tmp_path, technique)
    rc, msg = _render(evplp, jp, _block())
    assert rc == evplp.ERR_PARSE and "adaptive" in msg and technique in msg, (rc, msg)
    assert not (tmp_path / "noise.json").exists() and not (tmp_path / "iters.pfm").exists()


def test_a_valid_block_gets_past_validation(evplp, room, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_adaptive.py)")
    jp = _technique_file(room, tmp_path, "photonfam")
    rc_plain, msg_plain = _render(evplp, jp)
    rc, msg = _render(evplp, jp, _block())
    assert rc_plain < 0 and rc == rc_plain, (rc, msg, rc_plain, msg_plain)
    assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "adaptive" not in msg, msg
