"""The denoiser without a GPU: the two additive entry points (exported, bound, declared, refusing null handles), the parameter struct's size,
and the optional "denoise" block of the technique JSON -- validated completely before any group exists, so that a bad block costs no GPU
time, writes nothing and fails here."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
NEW = ("evplp_denoise", "evplp_group_denoise")


def _render(evplp, path, overrides=None):
    err = C.create_string_buffer(1024)
    rc = evplp.lib().evplp_render_json(str(path).encode(), overrides.encode() if overrides else None, 0, err, 1024)
    return rc, err.value.decode()


def test_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    # evplp_denoise_params: int32 levels, three floats, int32 reserved[4] -- 32 bytes, as the header declares it
    m = re.search(r"typedef struct evplp_denoise_params \{(.*?)\} evplp_denoise_params;", hdr, re.S)
    assert m, "evplp_denoise_params is not declared"
    fields = re.findall(r"\b(int32_t|float)\s+(\w+)(\[\d+\])?;", m.group(1))
    assert [f[1] for f in fields] == [f[0] for f in evplp.DenoiseParams._fields_], fields
    size = sum((4 * (int(f[2][1:-1]) if f[2] else 1)) for f in fields)
    assert C.sizeof(evplp.DenoiseParams) == size == 32
    L = evplp.lib()
    rgb = np.zeros((H, W, 3), np.float32)
    for p in ("", "group_"):
        assert getattr(L, f"evplp_{p}denoise")(None, 1.0, 1.0, 0, None, rgb.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_abi_version() == 5


class _NoC:
    """Stands in for the library: any C call fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"C call {name} made before the arguments were checked")


@pytest.mark.parametrize("cls", ["Context", "Group"])
def test_python_checks_levels_before_any_c_call(evplp, cls):
    obj = object.__new__(getattr(evplp, cls))
    obj._lib = _NoC(); obj._h = None; obj.W, obj.H = W, H
    for levels in (1.5, "5", True, None):
        with pytest.raises(ValueError):
            obj.denoise(0.1, levels=levels)


@pytest.fixture
def room(evplp, tmp_path):
    return evplp.synth_scene(str(tmp_path), "room", 600, 1, W, H)


NOISE = {"filename": "noise.json", "batchIterations": 1}
GOOD = {"filename": "denoised.pfm", "levels": 5, "sigmaLuminance": 4, "sigmaNormal": 128, "sigmaPosition": 0.01}


def _block(noise=True, **kw):
    b = dict(GOOD)
    for k, v in kw.items():
        if v is None:
            b.pop(k)
        else:
            b[k] = v
    out = {"denoise": b}
    if noise:
        out["noise"] = NOISE
    return json.dumps(out)


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


@pytest.mark.parametrize("technique", ["photonfam", "lvcphotonfam", "pt"])
def test_bad_denoise_blocks_are_refused_before_any_gpu_work(evplp, room, tmp_path, technique):
    jp = _technique_file(room, tmp_path, technique)
    cases = [
        (_block(noise=False), ["denoise", "noise"]),
        (_block(filename=None), ["denoise.filename"]),
        (_block(filename=3), ["denoise.filename"]),
        (_block(levels=0), ["denoise.levels"]),
        (_block(levels=11), ["denoise.levels"]),
        (_block(sigmaLuminance=-1), ["denoise.sigmaLuminance"]),
        (_block(sigmaNormal=-128), ["denoise.sigmaNormal"]),
        (_block(sigmaPosition=-0.01), ["denoise.sigmaPosition"]),
        (json.dumps({"denoise": 3, "noise": NOISE}), ["denoise"]),
        (json.dumps({"denoise": GOOD, "noise": NOISE, "frameMode": "cleareveryframe"}), ["denoise", "cleareveryframe"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    written = sorted(p.name for p in tmp_path.iterdir() if p.suffix in (".pfm", ".ppm", ".png", ".exr") or p.name == "noise.json")
    assert not (tmp_path / "denoised.pfm").exists() and not (tmp_path / "noise.json").exists(), written


@pytest.mark.parametrize("technique", ["photonfam", "pt"])
def test_a_valid_block_gets_past_validation(evplp, room, tmp_path, technique):
    import torch
    if torch.cuda.is_available():
        pytest.skip("with a GPU the run itself goes ahead (tests/test_gpu_denoise.py)")
    jp = _technique_file(room, tmp_path, technique)
    rc_plain, msg_plain = _render(evplp, jp)
    rc, msg = _render(evplp, jp, _block())
    assert rc_plain < 0 and rc == rc_plain, (rc, msg, rc_plain, msg_plain)
    assert rc not in (evplp.ERR_PARSE, evplp.ERR_IO) and "denoise" not in msg, msg
    rc, msg = _render(evplp, jp, json.dumps({"denoise": {"filename": "d.pfm"}, "noise": {"filename": "n.json"}}))
    assert rc == rc_plain, (rc, msg)
