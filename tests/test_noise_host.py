"""Per-pixel noise without a GPU: the eight additive entry points (exported, bound, declared, refusing null handles), the optional "noise" block
of the technique JSON -- validated completely before any group exists, so that a bad block costs no GPU time and fails here -- the Python
binding's argument checks, and the code objects of the noise kernels (zero scratch, no spills)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from test_kernel_resources import HIPCC, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
NEW = ("evplp_noise_track", "evplp_noise_fold", "evplp_noise_estimate", "evplp_noise_variance",
       "evplp_group_noise_track", "evplp_group_noise_fold", "evplp_group_noise_estimate", "evplp_group_noise_variance")


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
    out = (C.c_double * 3)()
    rgb = np.zeros((H, W, 3), np.float32)
    L = evplp.lib()
    for p in ("", "group_"):
        assert getattr(L, f"evplp_{p}noise_track")(None, 1, None) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}noise_fold")(None, 1) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}noise_estimate")(None, 1.0, 1.0, 0, C.byref(out)) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}noise_variance")(None, 1.0, rgb.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_noise_kernels_have_no_scratch_and_no_spills():
    table = kernel_table("kernels_stats.hip")
    hits = {k: v for k, v in table.items() if "noise_" in k}
    for kind in ("noise_fold_kernelILb0", "noise_fold_kernelILb1", "noise_pool_kernel", "noise_rows_kernel", "noise_variance_kernel"):
        assert sum(kind in k for k in hits) == 1, (kind, sorted(hits))
    for k, t in hits.items():
        assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (k, t)


class _NoC:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} made before the arguments were checked")


@pytest.mark.parametrize("cls", ["Context", "Group"])
def test_python_checks_arguments_before_any_c_call(evplp, cls):
    obj = object.__new__(getattr(evplp, cls))
    obj._lib = _NoC(); obj._h = None; obj.W, obj.H = W, H
    mask = np.ones((H, W, 3), np.uint8)
    for on, m in [(True, mask.astype(np.float32)), (True, np.ones((H, W), np.uint8)), (True, np.ones((H, W + 1, 3), np.uint8)),
                  (False, mask), ("yes", None), (True, [[1]])]:
        with pytest.raises(ValueError):
            obj.noise_track(on, m)
    for k in (0, -3, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            obj.noise_fold(k)


@pytest.fixture
def room(evplp, tmp_path):
    jp = evplp.synth_scene(str(tmp_path), "room", 600, 1, W, H)
    m = np.ones((H, W, 3), np.float32); m[:8] = 0.0
    evplp.save_image(str(tmp_path / "mask.png"), m)
    evplp.save_image(str(tmp_path / "small_mask.png"), np.ones((H - 2, W, 3), np.float32))
    return jp


GOOD = {"batchIterations": 2, "everyIterations": 4, "everyMs": 50, "stopRelMse": 0.01, "mask": "mask.png", "filename": "noise.json",
        "varianceFilename": "var.pfm"}


def _block(**kw):
    b = dict(GOOD)
    for k, v in kw.items():
        if v is None:
            b.pop(k)
        else:
            b[k] = v
    return json.dumps({"noise": b})


@pytest.mark.parametrize("technique", ["photonfam", "lvcphotonfam", "pt"])
def test_bad_noise_blocks_are_refused_before_any_gpu_work(evplp, room, tmp_path, technique):
    root = json.load(open(room))
    if technique == "pt":
        root["pt"] = {"rngOffset": 0, "numMaxIteration": 2, "timeLimitMs": 1e9, "frameMode": "accumulate", "outputFilename": "pt.pfm",
                      "statFilename": "pt.json", "useJitter": True, "useStat": True, "numSamplePerPixel": 1, "numMaxBounces": 3}
        root.pop("photonfam")
    elif technique == "lvcphotonfam":
        root["lvcphotonfam"] = root.pop("photonfam")
    jp = tmp_path / f"{technique}.json"
    jp.write_text(json.dumps(root))
    cases = [
        (_block(filename=None), evplp.ERR_PARSE, ["noise.filename"]),
        (_block(batchIterations=0), evplp.ERR_PARSE, ["noise.batchIterations"]),
        (_block(batchIterations=-2), evplp.ERR_PARSE, ["noise.batchIterations"]),
        (_block(batchIterations="2"), evplp.ERR_PARSE, ["noise.batchIterations"]),
        (_block(everyIterations=0), evplp.ERR_PARSE, ["noise.everyIterations"]),
        (_block(everyIterations=5), evplp.ERR_PARSE, ["noise.everyIterations", "multiple"]),
        (_block(everyMs=-5), evplp.ERR_PARSE, ["noise.everyMs"]),
        (_block(stopRelMse=-1e-3), evplp.ERR_PARSE, ["noise.stopRelMse"]),
        (_block(varianceFilename=3), evplp.ERR_PARSE, ["noise.varianceFilename"]),
        (json.dumps({"noise": 3}), evplp.ERR_PARSE, ["noise"]),
        (json.dumps({"noise": GOOD, "frameMode": "cleareveryframe"}), evplp.ERR_PARSE, ["noise", "cleareveryframe"]),
        (_block(mask="missing.png"), evplp.ERR_IO, ["noise.mask", "missing.png"]),
        (_block(mask="small_mask.png"), evplp.ERR_PARSE, ["96 x 62", "96 x 64"]),
    ]
    for overrides, code, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == code, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    assert not (tmp_path / "noise.json").exists() and not (tmp_path / "var.pfm").exists()


def test_a_valid_block_gets_past_validation(evplp, room):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_noise.py)")
    rc_plain, msg_plain = _render(evplp, room)
    rc, msg = _render(evplp, room, _block())
    assert rc_plain < 0 and rc == rc_plain, (rc, msg, rc_plain, msg_plain)
    assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "noise" not in msg, msg
    rc, msg = _render(evplp, room, json.dumps({"noise": {"filename": "n.json"}}))
    assert rc == rc_plain, (rc, msg)
