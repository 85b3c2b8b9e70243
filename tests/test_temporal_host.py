"""Temporal accumulation without a GPU: the additive entry points (exported, bound, declared, refusing null handles), the two structs' sizes
and field order, the ABI version, and evplp_project_points against its numpy fp32 restatement bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_restate as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEW = ("evplp_temporal_enable", "evplp_temporal_reset", "evplp_denoise_temporal", "evplp_temporal_download", "evplp_project_points",
       "evplp_group_temporal_enable", "evplp_group_temporal_reset", "evplp_group_denoise_temporal", "evplp_group_temporal_download")

CAMERAS = [
    dict(origin=(0.0, -8.0, 3.0), lookat=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), fovy=0.9),
    dict(origin=(2.5, 1.25, -3.0), lookat=(0.1, 0.4, 0.3), up=(0.0, 1.0, 0.0), fovy=0.6),
    dict(origin=(-4.0, 3.0, 6.5), lookat=(1.0, -2.0, 0.5), up=(0.2, 0.1, 1.0), fovy=1.3),
]
SIZES = [(96, 64), (90, 50)]


def test_entry_points_are_exported_bound_declared_and_refuse_null_handles(evplp):
    lib = C.CDLL(evplp.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in evplp._SIGNATURES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    L = evplp.lib()
    rgb = np.zeros((64, 96, 4), F)
    assert L.evplp_temporal_enable(None, 1) == evplp.ERR_INVALID
    assert L.evplp_temporal_reset(None) == evplp.ERR_INVALID
    assert L.evplp_denoise_temporal(None, 1.0, 1.0, 0, None, None, rgb.ctypes.data, None) == evplp.ERR_INVALID
    assert L.evplp_temporal_download(None, 0, rgb.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_group_temporal_enable(None, 1) == evplp.ERR_INVALID
    assert L.evplp_group_temporal_reset(None) == evplp.ERR_INVALID
    assert L.evplp_group_denoise_temporal(None, 1.0, 1.0, 0, None, None, rgb.ctypes.data, None) == evplp.ERR_INVALID
    assert L.evplp_group_temporal_download(None, 0, rgb.ctypes.data) == evplp.ERR_INVALID
    cam = evplp._camera((0, 0, 0), (0, 0, -1), (0, 1, 0), 0.8, 1.5)
    p = np.zeros((2, 3), F)
    assert L.evplp_project_points(None, 96, 64, p.ctypes.data, 2, p.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_project_points(C.byref(cam), 96, 64, None, 2, p.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_project_points(C.byref(cam), 96, 64, p.ctypes.data, 2, None) == evplp.ERR_INVALID
    assert L.evplp_project_points(C.byref(cam), 0, 64, p.ctypes.data, 2, p.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_project_points(C.byref(cam), 96, 64, p.ctypes.data, -1, p.ctypes.data) == evplp.ERR_INVALID
    assert L.evplp_project_points(C.byref(cam), 96, 64, None, 0, None) == evplp.OK
    assert L.evplp_abi_version() == 5
    assert "#define EVPLP_ABI_VERSION 5" in re.sub(r"[ \t]+", " ", hdr)
    types = open(os.path.join(ROOT, "evplp_amd", "csrc", "evplp_types.h")).read()
    assert "__host__ __device__ inline bool project_point(const CamBasis &cam, int32_t W, int32_t H, const float p[3], float out[3])" in types


def test_structs_have_the_declared_size_and_field_order(evplp):
    hdr = open(os.path.join(ROOT, "include", "evplp.h")).read()
    sizes = {"int32_t": 4, "float": 4, "int64_t": 8}
    for name, mirror, want in (("evplp_temporal_params", evplp.TemporalParams, 32), ("evplp_temporal_info", evplp.TemporalInfo, 40)):
        m = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S)
        assert m, name
        fields = []
        for ty, names in re.findall(r"\b(int32_t|int64_t|float)\s+([^;]+);", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)):
            for nm in names.split(","):
                mm = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
                fields.append((mm.group(1), sizes[ty] * int(mm.group(2) or 1)))
        assert [f[0] for f in fields] == [f[0] for f in mirror._fields_], (name, fields)
        assert sum(f[1] for f in fields) == C.sizeof(mirror) == want, (name, fields)
    assert [getattr(evplp, "TEMPORAL_" + n) for n in ("HISTORY_U", "HISTORY_POS", "HISTORY_NRM", "PREV_POS", "PREV_NRM", "DEBUG_HIT")] == \
        [int(re.search(r"#define EVPLP_TEMPORAL_" + n + r"\s+(\d+)", hdr).group(1)) for n in ("HISTORY_U", "HISTORY_POS", "HISTORY_NRM", "PREV_POS", "PREV_NRM", "DEBUG_HIT")]


@pytest.mark.parametrize("cls", ["Context", "Group"])
def test_python_checks_max_history_before_any_c_call(evplp, cls):
    class NoC:
        def __getattr__(self, name):
            raise AssertionError(f"C call {name} made before the arguments were checked")
    obj = object.__new__(getattr(evplp, cls))
    obj._lib = NoC(); obj._h = None; obj.W, obj.H = 96, 64
    for mh in (1.5, "4", True, None):
        with pytest.raises(ValueError):
            obj.denoise_temporal(0.1, max_history=mh)


@pytest.mark.parametrize("W, H", SIZES)
@pytest.mark.parametrize("cam", CAMERAS)
def test_project_points_matches_the_restatement_bit_for_bit_and_finds_the_pixel_centres(evplp, cam, W, H):
    aspect = W / H
    basis = tr.camera_basis(cam["origin"], cam["lookat"], cam["up"], cam["fovy"], aspect)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rng = np.random.default_rng(5)
    t = rng.uniform(0.2, 40.0, size=xs.shape).astype(F)
    pts = tr.primary_points(basis, W, H, xs, ys, t)
    got = evplp.project_points(cam["origin"], cam["lookat"], cam["up"], cam["fovy"], aspect, W, H, pts.reshape(-1, 3)).reshape(H, W, 3)
    want, ok = tr.project(basis, W, H, pts)
    assert ok.all()
    assert got.tobytes() == want.tobytes()
    # the pixel centres, to 1e-3 pixel; the depth is the ray parameter (the direction's view-space depth is 1)
    assert np.abs(got[..., 0] - xs).max() < 1e-3 and np.abs(got[..., 1] - ys).max() < 1e-3
    assert np.abs(got[..., 2] / t - 1).max() < 1e-5
    # points anywhere, some behind the eye: reported as such, bit for bit again
    far = (np.asarray(cam["origin"], F) + rng.normal(0, 5.0, size=(4096, 3))).astype(F)
    far[0] = np.asarray(cam["origin"], F)                                   # the eye itself: depth 0
    got = evplp.project_points(cam["origin"], cam["lookat"], cam["up"], cam["fovy"], aspect, W, H, far)
    want, ok = tr.project(basis, W, H, far)
    assert got.tobytes() == want.tobytes()
    assert (~ok).sum() > 1000 and ok.sum() > 1000
    assert (got[~ok, 2] <= 0).all() and (got[~ok, :2] == 0).all() and (got[ok, 2] > 0).all()


def _render(evplp, path, overrides=None):
    err = C.create_string_buffer(1024)
    rc = evplp.lib().evplp_render_json(str(path).encode(), overrides.encode() if overrides else None, 0, err, 1024)
    return rc, err.value.decode()


@pytest.mark.parametrize("technique", ["photonfam", "lvcphotonfam", "pt"])
def test_bad_temporal_and_rng_advance_blocks_are_refused_before_any_gpu_work(evplp, tmp_path, technique):
    import json
    from test_denoise_host import GOOD, NOISE, _technique_file
    room = evplp.synth_scene(str(tmp_path), "room", 600, 1, 96, 64)
    jp = _technique_file(room, tmp_path, technique)
    ident = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    anim = {"frames": 2, "tracks": [{"mesh": 0, "matrices": [ident, ident]}]}
    base = {"numMaxIteration": 2, "timeLimitMs": 1e9, "noise": NOISE}

    def block(temporal, animation=anim, **kw):
        o = dict(base, denoise=dict(GOOD, temporal=temporal), **kw)
        if animation is not None:
            o["animation"] = animation
        return json.dumps(o)
    cases = [
        (block({}, animation=None), ["denoise.temporal", "animation"]),
        (block(3), ["denoise.temporal"]),
        (block({"maxHistroy": 4}), ["denoise.temporal.maxHistroy"]),
        (block({"maxHistory": 0}), ["denoise.temporal.maxHistory"]),
        (block({"maxHistory": 1025}), ["denoise.temporal.maxHistory"]),
        (block({"maxHistory": 2.5}), ["denoise.temporal.maxHistory"]),
        (block({"normalCos": 0}), ["denoise.temporal.normalCos"]),
        (block({"normalCos": 1.5}), ["denoise.temporal.normalCos"]),
        (block({"normalCos": "0.9"}), ["denoise.temporal.normalCos"]),
        (json.dumps(dict(base, animation=dict(anim, rngAdvance=-1))), ["animation.rngAdvance"]),
        (json.dumps(dict(base, animation=dict(anim, rngAdvance=1.5))), ["animation.rngAdvance"]),
        (json.dumps(dict(base, animation=dict(anim, rngAdvance="2"))), ["animation.rngAdvance"]),
    ]
    for overrides, needles in cases:
        rc, msg = _render(evplp, jp, overrides)
        assert rc == evplp.ERR_PARSE, (overrides, rc, msg)
        for n in needles:
            assert n in msg, (overrides, msg)
    assert not [p.name for p in tmp_path.iterdir() if p.suffix == ".pfm" or p.name == "noise.json"]
