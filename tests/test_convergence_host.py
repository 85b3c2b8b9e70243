"""Error against a reference image without a GPU: the four additive entry points (exported, bound, refusing null handles), the optional
"convergence" block of the technique JSON -- validated completely before any group exists, so that a bad block costs no GPU time and
fails here -- the Python binding's argument checks, and the code object of frame_error_kernel (zero scratch, no spills)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from test_kernel_resources import HIPCC, kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
NEW = ("evplp_set_error_reference", "evplp_frame_error", "evplp_group_set_error_reference", "evplp_group_frame_error")


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
    L = evplp.lib()
    assert L.evplp_set_error_reference(None, None, None) == evplp.ERR_INVALID
    assert L.evplp_frame_error(None, 1.0, 1.0, 1.0, 0, 0, C.byref(out)) == evplp.ERR_INVALID
    assert L.evplp_group_set_error_reference(None, None, None) == evplp.ERR_INVALID
    assert L.evplp_group_frame_error(None, 1.0, 1.0, 1.0, 0, 0, C.byref(out)) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_frame_error_kernel_has_no_scratch_and_no_spills():
    table = kernel_table("kernels_stats.hip")
    hits = [k for k in table if "frame_error_kernel" in k]
    assert len(hits) == 1, sorted(table)
    t = table[hits[0]]
    assert t["private_segment_fixed_size"] == 0 and t["vgpr_spill_count"] == 0 and t["sgpr_spill_count"] == 0, (hits[0], t)


class _NoC:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} made before the arguments were checked")


@pytest.mark.parametrize("cls", ["Context", "Group"])
def test_python_checks_shapes_and_dtypes_before_any_c_call(evplp, cls):
    obj = object.__new__(getattr(evplp, cls))
    obj._lib = _NoC(); obj._h = None; obj.W, obj.H = W, H
    ref = np.zeros((H, W, 3), np.float32)
    mask = np.ones((H, W, 3), np.uint8)
    bad = [
        (ref.astype(np.float64), None),            # dtype
        (np.zeros((W, H, 3), np.float32), None),   # transposed
        (np.zeros((H, W, 4), np.float32), None),   # RGBA
        (np.zeros((H - 1, W, 3), np.float32), None),
        (ref, mask.astype(np.float32)),            # mask dtype
        (ref, np.ones((H, W), np.uint8)),          # single-channel mask
        (ref, np.ones((H, W + 1, 3), np.uint8)),
        (None, mask),                              # a mask without a reference
        ([[0.0]], None),
    ]
    for rgb, m in bad:
        with pytest.raises(ValueError):
            obj.set_error_reference(rgb, m)


@pytest.fixture
def room(evplp, tmp_path):
    jp = evplp.synth_scene(str(tmp_path), "room", 600, 1, W, H)
    evplp.save_image(str(tmp_path / "ref.pfm"), np.full((H, W, 3), 0.25, np.float32))
    evplp.save_image(str(tmp_path / "small.pfm"), np.full((H, W - 1, 3), 0.25, np.float32))
    m = np.ones((H, W, 3), np.float32); m[:8] = 0.0
    evplp.save_image(str(tmp_path / "mask.png"), m)
    evplp.save_image(str(tmp_path / "small_mask.png"), np.ones((H - 2, W, 3), np.float32))
    return jp


GOOD = {"reference": "ref.pfm", "mask": "mask.png", "everyIterations": 2, "everyMs": 50, "stopRelMse": 0.01, "filename": "curve.json"}


def _block(**kw):
    b = dict(GOOD)
    for k, v in kw.items():
        if v is None:
            b.pop(k)
        else:
            b[k] = v
    return json.dumps({"convergence": b})


@pytest.mark.parametrize("technique", ["photonfam", "pt"])
def test_bad_convergence_blocks_are_refused_with_the_key_or_sizes(evplp, room, tmp_path, technique):
    root = json.load(open(room))
    if technique == "pt":
        root["pt"] = {"rngOffset": 0, "numMaxIteration": 2, "timeLimitMs": 1e9, "frameMode": "accumulate", "outputFilename": "pt.pfm",
                      "statFilename": "pt.json", "useJitter": True, "useStat": True, "numSamplePerPixel": 1, "numMaxBounces": 3}
        root.pop("photonfam")
    jp = tmp_path / f"{technique}.json"
    jp.write_text(json.dumps(root))
    cases = [
        (_block(reference=None), evplp.ERR_PARSE, ["convergence.reference"]),
        (_block(filename=None), evplp.ERR_PARSE, ["convergence.filename"]),
        (_block(everyIterations=0), evplp.ERR_PARSE, ["convergence.everyIterations"]),
        (_block(everyMs=-5), evplp.ERR_PARSE, ["convergence.everyMs"]),
        (_block(stopRelMse=-1e-3), evplp.ERR_PARSE, ["convergence.stopRelMse"]),
        (json.dumps({"convergence": 3}), evplp.ERR_PARSE, ["convergence"]),
        (_block(reference="missing.pfm"), evplp.ERR_IO, ["convergence.reference", "missing.pfm"]),
        (_block(mask="missing.png"), evplp.ERR_IO, ["convergence.mask", "missing.png"]),
        (_block(reference="small.pfm"), evplp.ERR_PARSE, ["95 x 64", "96 x 64"]),
        (_block(mask="small_mask.png"), evplp.ERR_PARSE, ["96 x 62", "96 x 64"]),
    ]
    for overrides, code, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == code, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    assert not (tmp_path / "curve.json").exists()


def test_a_valid_block_gets_past_validation(evplp, room):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_convergence.py)")
    rc_plain, msg_plain = _render(evplp, room)
    rc, msg = _render(evplp, room, _block())
    assert rc_plain < 0 and rc == rc_plain, (rc, msg, rc_plain, msg_plain)
    assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "convergence" not in msg, msg
    rc, msg = _render(evplp, room, _block(mask=None, everyMs=None, stopRelMse=None))
    assert rc == rc_plain, (rc, msg)
