"""Batched path tracing without a GPU: the four additive entry points (exported, bound, declared, refusing null handles; the ABI version
unchanged), the contract of evplp_path_trace_batch in the header, and the pt technique's build-only key "samplesPerCall" -- validated
completely before any group exists, so that a bad value costs no GPU time and fails here with a parse error naming the key."""
import ctypes as C
import json
import os
import re

import pytest

from test_adaptive_host import GOOD, NOISE, _render, _technique_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evplp_path_trace_batch", "evplp_path_trace_batch_scratch", "evplp_group_path_trace_batch", "evplp_group_path_trace_batch_scratch")
KEY = "samplesPerCall"


def _header():
    return open(os.path.join(ROOT, "include", "evplp.h")).read()


def test_new_entry_points_are_exported_bound_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = _header()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    cam = (C.c_float * 3)(0, 0, 0); jit = (C.c_float * 2)(0, 0); seed = (C.c_uint32 * 1)(0)
    for p in ("", "group_"):
        assert getattr(L, f"evplp_{p}path_trace_batch")(None, cam, 1, jit, seed, 3) == evplp.ERR_INVALID
        assert getattr(L, f"evplp_{p}path_trace_batch_scratch")(None, 1 << 20) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    for cls in (evplp.Context, evplp.Group):
        assert callable(getattr(cls, "path_trace_batch")) and callable(getattr(cls, "path_trace_batch_scratch"))


def test_the_header_states_the_contract():
    hdr = _header()
    k = hdr.index("int evplp_path_trace_batch(")
    doc = re.sub(r"\s*\n\s*\*\s*", " ", hdr[hdr.rindex("/* S complete iterations", 0, k):k])
    for needle in ("evplp_primary(ctx, jitters + 2 s, 0); evplp_path_trace(ctx, camera_pos, rng_seeds[s], max_bounces, 1)",
                   "bit-identical to the sequence", "in increasing s", "out + r0 + r1 is not out + (r0 + r1)",
                   "(float)((double)R * ((double)(N + samples) / (double)n_t))", "N advances by samples",
                   "evplp_primary at jitters[samples - 1], flags 0", "EVPLP_BUF_LIGHT, retired tiles", "only the closing pass's jitter",
                   "sums of the sequence's per-call figures", "evplp_path_trace_batch_scratch", "changes no bit",
                   "samples < 1 or > 64", "evplp_adaptive_enable", "4096 B"):
        assert needle in doc, needle
    assert "batched path tracing" in hdr                                 # the memory table's row


@pytest.fixture
def room(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, 96, 64)


def test_bad_values_are_refused_before_any_gpu_work(evplp, room, tmp_path):
    jp = _technique_file(room, tmp_path, "pt")
    noise4 = dict(NOISE, batchIterations=4, everyIterations=4)
    cases = [
        ({KEY: 0}, [KEY]),
        ({KEY: 65}, [KEY]),
        ({KEY: -3}, [KEY]),
        ({KEY: "4"}, [KEY]),
        ({KEY: 4, "frameMode": "cleareveryframe"}, [KEY, "cleareveryframe"]),
        ({KEY: 4, "writeEveryFrame": True}, [KEY, "writeEveryFrame"]),
        ({KEY: 4, "noise": NOISE}, [KEY, "noise.batchIterations", "multiple"]),                     # 2 is not a multiple of 4
        ({KEY: 3, "noise": noise4}, [KEY, "noise.batchIterations", "multiple"]),
        ({KEY: 4, "noise": NOISE, "adaptiveSampling": GOOD}, [KEY, "noise.batchIterations", "adaptiveSampling", "multiple"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, json.dumps(overrides))
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    for f in ("noise.json", "iters.pfm", "pt.pfm"):
        assert not (tmp_path / f).exists(), f


def test_valid_values_get_past_validation(evplp, room, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_pt_batch.py)")
    jp = _technique_file(room, tmp_path, "pt")
    rc_plain, msg_plain = _render(evplp, jp)
    for overrides in ({KEY: 1, "frameMode": "cleareveryframe", "writeEveryFrame": True}, {KEY: 1, "noise": dict(NOISE, batchIterations=3, everyIterations=3)},
                      {KEY: 2, "noise": NOISE, "adaptiveSampling": GOOD}, {KEY: 64}):
        rc, msg = _render(evplp, jp, json.dumps(overrides))
        assert rc_plain < 0 and rc == rc_plain, (overrides, rc, msg, rc_plain, msg_plain)
        assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and KEY not in msg, msg
